"""CPU test (no GPU) that pins what the launchers DO with a call: for every launch of every case the choice its family's
chooser returns (csrc/qvc_select.h) -- kernel instantiation, tile, grid, LDS size --, recorded by the CPU twin's selecting
backend (tools/emu_twin.cpp: SelectBackend, qvc_emu_launch_trace), equals tests/golden/launch_trace.json.  That file was
written by tests/golden/make_golden_launch_trace.py from the selection rules as they were moved out of the device headers,
before the dispatchers were rewritten; tests/test_path_trace_host.py shows that the GPU is handed the same launches, this
shows that each of them gets the same kernel, tile and grid.
"""
import ctypes
import importlib
import importlib.util
import json
import os

import pytest

from helpers import ROOT
from live_common import built  # noqa: F401


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_launch_trace", os.path.join(ROOT, "tests", "golden", "make_golden_launch_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def trace(built):
    """(generator module, {case: [(kind, [words])]}, {kind: [word names]}) -- recorded once for the tests below."""
    gen = _generator()
    twin = ctypes.CDLL(importlib.import_module("quickvc_official_amd.build").build_emu_twin())
    full, names = gen.collect_full(twin)
    return gen, full, names


def test_every_choice_is_the_golden_one(trace):
    gen, full, _names = trace
    want = json.load(open(gen.PATH))
    got = gen.compress(full)
    assert sorted(got) == sorted(want)
    for case in sorted(want):
        g_names, w_names = got[case]["names"].split(" "), want[case]["names"].split(" ")
        g_hash, w_hash = got[case]["hashes"].split(" "), want[case]["hashes"].split(" ")
        assert len(w_names) == len(w_hash)
        for i, (gn, wn, gh, wh) in enumerate(zip(g_names, w_names, g_hash, w_hash)):
            assert (gn, gh) == (wn, wh), f"{case}: call {i} is {gn} {gh}, the golden one {wn} {wh} (make_golden_launch_trace.py --dump shows the fields)"
        assert len(g_names) == len(w_names), f"{case}: {len(g_names)} calls, the golden file has {len(w_names)}"


def test_every_choice_is_instantiated_and_fits_the_lds(trace):
    """Every choice in the trace is accepted (status 0), names a template tuple the library instantiates (the family's
    *_built predicate, evaluated by the twin next to the chooser) and asks for at most 160 KiB of LDS."""
    gen, full, names = trace
    picked = gen.choices(full, names)
    assert len(picked) > 1000 and {kind for _c, kind, _r in picked} == set(gen.FAMILY_KINDS)
    for case, kind, r in picked:
        assert r["c.status"] == 0, (case, kind, r)
        assert r["built"] == 1, (case, kind, r)
        assert 0 <= r["c.lds"] <= 160 * 1024, (case, kind, r)
        assert r["c.block"] % 64 == 0 and 64 <= r["c.block"] <= 1024 and min(r["c.grid[0]"], r["c.grid[1]"], r["c.grid[2]"]) >= 1, (case, kind, r)


def test_the_table_covers_every_rule_in_both_directions(trace):
    gen, full, names = trace
    gen.check_coverage(full, names)
