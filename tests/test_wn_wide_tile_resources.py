"""CPU check of the 64-frame WaveNet stack tile (qvc_wn2_impl.h, NF = 5): hipcc's resource remarks, kept by build.py
next to the objects, must show no scratch memory and three waves per SIMD (one 12-wave workgroup per CU, <= 168
VGPRs) for every instantiation of the tile -- both operand types, with and without the fused post conv."""
import os
import re
import sys

import pytest

from helpers import ROOT


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from quickvc_official_amd import lib as L
    return L.load_library()


def _remarks(path):
    """{function name: {"vgpr": n, "scratch": n, "occupancy": n}} from one remarks file"""
    out, name = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        for key, pat in (("vgpr", r"\bVGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def test_wide_wn_tile_has_no_scratch_and_three_waves_per_simd(built):
    rem = _remarks(os.path.join(ROOT, "quickvc-official_amd", "csrc", "_obj", "qvc_wn2.remarks.txt"))
    # wn_stack2_kernel<T, KS 6, TAPS 5, PM, NF 5, RING>
    wide = {n: r for n, r in rem.items() if re.search(r"wn_stack2_kernelIDF16[_b]Li6ELi5ELi[01]ELi5ELi\d+E", n)}
    assert len(wide) == 4, sorted(rem)
    for n, r in wide.items():
        assert r["scratch"] == 0, (n, r)
        assert r["occupancy"] >= 3 and r["vgpr"] <= 168, (n, r)
