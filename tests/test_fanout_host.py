"""CPU tests (no GPU) of the fan-out path -- R output rows from U <= R encoded sources (include/qvc.h:
qvc_infer_fanout_ragged): the C ABI's surface, sizes and error codes, the host-side row map of the CLI, the unchanged
plan, the frozen host emulation, and the resource remarks of the kernels the feature adds."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from helpers import ROOT


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from quickvc_official_amd import lib as L
    return L.load_library()


def _cfg(**over):
    import quickvc_official_amd as q
    from quickvc_official_amd import lib as L
    model = q.SynthesizerTrn(641, 32, **q.MINI_MODEL_CONFIG)
    cfg = L.make_config(model.model_config)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def test_exports_and_sizes(built):
    for name in ("qvc_fanout_workspace_bytes", "qvc_infer_fanout_ragged", "qvc_infer_fanout_ragged_fm"):
        assert hasattr(built, name), name
    assert built.qvc_abi_version() == 8
    cfg = _cfg()
    for U, R, T in ((1, 1, 2), (3, 7, 37), (1, 32, 250), (32, 32, 250), (5, 65, 33)):
        plain = int(built.qvc_workspace_bytes(ctypes.byref(cfg), R, T))
        fan = int(built.qvc_fanout_workspace_bytes(ctypes.byref(cfg), U, R, T))
        assert plain > 0 and fan >= plain + 4 * R, (U, R, T, plain, fan)       # the per-row length array follows the workspace
        assert fan % 256 == 0 and fan - plain <= 4 * R + 256


def test_error_codes(built):
    cfg, bad = _cfg(), _cfg(n_flows=3)
    q = built.qvc_fanout_workspace_bytes
    assert q(ctypes.byref(cfg), 0, 4, 37) == -1                       # no source
    assert q(ctypes.byref(cfg), 5, 4, 37) == -1                       # more sources than rows
    assert q(ctypes.byref(cfg), 2, 4, 1) == -1                        # frames <= 1, as qvc_workspace_bytes
    assert q(None, 2, 4, 37) == -1
    assert q(ctypes.byref(bad), 2, 4, 37) == -2                       # the code comes back as the value
    need = int(q(ctypes.byref(cfg), 3, 7, 37))
    assert need > 0
    # None of these calls gets as far as a launch: every pointer is checked (never followed) on the host first.
    p = 1 << 20                                                        # any 256-byte aligned non-null address
    for fn in (built.qvc_infer_fanout_ragged, built.qvc_infer_fanout_ragged_fm):
        def call(cfg_=cfg, blob=p, unit=p, frames=p, src=p, g=p, noise=p, out=p, U=3, R=7, T=37, ws=p, n=need):
            return fn(ctypes.byref(cfg_) if cfg_ is not None else None, blob, unit, frames, src, g, noise, out, U, R, T, ws, n, None)
        assert call(U=0) == -1 and call(U=8) == -1 and call(R=0, U=0) == -1 and call(T=1) == -1
        for null in ("blob", "unit", "frames", "src", "g", "noise", "out", "ws"):
            assert call(**{null: None}) == -1, null
        assert call(cfg_=None) == -1
        assert call(cfg_=bad) == -2
        assert call(n=need - 1) == -5                                  # one byte short
        assert call(n=int(built.qvc_workspace_bytes(ctypes.byref(cfg), 7, 37))) == -5   # the plain workspace has no room for the lengths
        assert call(ws=p + 4) == -1                                    # misaligned workspace, as the other entry points


def test_fanout_rows():
    from quickvc_official_amd.convert import fanout_rows
    assert fanout_rows(["a", "b", "a", "c", "b", "a"]) == (["a", "b", "c"], [0, 1, 0, 2, 1, 0])
    paths = [f"u{i}.npy" for i in range(9)]
    assert fanout_rows(paths) == (paths, list(range(9)))              # all distinct: the identity map
    assert fanout_rows(["x.npy"] * 5) == (["x.npy"], [0] * 5)
    assert fanout_rows([]) == ([], [])
    uniq, src = fanout_rows(["b", "b", "a", "b"])
    assert [uniq[s] for s in src] == ["b", "b", "a", "b"]


def test_plan_does_not_change_with_repeated_sources(built, tmp_path):
    """rank_plan sees lines, not sources: on a list with repeated sources it returns what plan_batches gives for the
    lines' lengths, for every rank -- the fan-out happens inside a planned batch."""
    from quickvc_official_amd import convert as cli
    from quickvc_official_amd.dist import shard_indices
    rng = np.random.RandomState(3)
    src_len = [int(v) for v in rng.randint(20, 90, size=12)]
    for i, n in enumerate(src_len):
        np.save(str(tmp_path / f"u{i:02d}.npy"), np.zeros((n, 256), dtype=np.float32))
    lines = [int(v) for v in rng.randint(0, 12, size=40)]
    items = [(f"o{k:02d}", str(tmp_path / f"u{s:02d}.npy"), f"spk{k % 4}.wav") for k, s in enumerate(lines)]
    want_len = [src_len[s] for s in lines]
    for rank, world in ((0, 1), (0, 2), (1, 2)):
        lengths, mine, batches = cli.rank_plan(items, rank, world, 8)
        assert lengths == want_len
        assert mine == shard_indices(len(items), rank, world, want_len)
        assert batches == [[mine[i] for i in idxs] for idxs in cli.plan_batches([want_len[i] for i in mine], 8)]
    _l, mine, batches = cli.rank_plan(items, 0, 1, 8)
    assert sorted(i for b in batches for i in b) == list(range(40))
    # ... and the map of a planned batch names each of its sources once
    saved = 0
    for b in batches:
        uniq, src = cli.fanout_rows([items[i][1] for i in b])
        assert len(set(uniq)) == len(uniq) and [uniq[s] for s in src] == [items[i][1] for i in b]
        saved += len(b) - len(uniq)
    assert saved > 0


def test_frozen_emulation_builds_and_loads_without_the_new_symbols(built):
    """oracle/qvc_emu.cpp implements the backend contract as it was: it builds against the new headers unchanged, does
    not state kFanout, and lib.declare() asks it for none of the new symbols."""
    import emu
    from quickvc_official_amd import lib as L
    emulib = emu.load_emu()
    assert not hasattr(emulib, "qvc_emu_infer_fanout_ragged")
    L.declare(emulib, prefix="qvc_emu")                                # must not look up what the library does not have
    src = open(os.path.join(ROOT, "oracle", "qvc_emu.cpp")).read()
    assert "kFanout" not in src and "sample_rows" not in src
    info_e, info_h = (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 8)()
    cfg = _cfg()
    assert emulib.qvc_emu_plan_flags(ctypes.byref(cfg), info_e) == 0 and built.qvc_plan_info(ctypes.byref(cfg), info_h) == 0
    assert list(info_e) == list(info_h)


def _remarks(name):
    """{mangled kernel name: scratch bytes per lane} of one translation unit"""
    out, cur = {}, None
    for line in open(os.path.join(ROOT, "quickvc-official_amd", "csrc", "_obj", name + ".remarks.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            out[cur] = int(m.group(1))
    return out


def test_new_kernels_use_no_scratch(built):
    """The statistics epilogue (EPI_STATS = 4: conv_mfma_kernel<T, MF, NF, 4, 4, false>) exists for the paired-row
    layouts MF 2 / 4 / 6 in every tile the launcher can pick, in both operand types, and none of them -- nor
    sample_rows_kernel -- spills."""
    want = {(2, 2), (2, 4), (2, 5), (2, 8), (2, 10), (4, 2), (4, 4), (4, 5), (4, 8), (4, 10), (6, 2), (6, 4), (6, 5)}
    for unit in ("qvc_conv_f16", "qvc_conv_bf16"):
        got = set()
        for name, scratch in _remarks(unit).items():
            m = re.search(r"conv_mfma_kernelIDF16[_b]Li(\d+)ELi(\d+)ELi4ELi4ELb0EEE", name)
            if m:
                assert scratch == 0, (name, scratch)
                got.add((int(m.group(1)), int(m.group(2))))
        assert got == want, (unit, sorted(want ^ got))
    small = {n: s for n, s in _remarks("qvc_small").items() if "sample_rows_kernel" in n}
    assert len(small) == 1 and list(small.values()) == [0], small
