"""The memory-contract helper (tests/memguard.py) and the property it demands, on the CPU (no GPU needed).

Two halves.  The checker itself: a byte written just outside a payload is reported with its side and distance, writes
inside are not, and a byte in an alignment gap of a workspace is found -- the analogue of the comparator self-tests in
tests/test_step_window.py.  And the path as designed: the host emulation (oracle/qvc_emu.cpp, the same Path<> over the
same packed blob) run from a workspace and an output filled with 0x00, 0x3C and 0xFF, with NaN in the padding of unit and
noise, gives bit-identical results and leaves the bytes that lie in no workspace buffer alone.  A failure of
tests/test_gpu_memory_contract.py is therefore a kernel's, not the design's.
"""
import pytest
import torch

import emu as E
import memguard as M
from helpers import load_case, regenerate


# ------------------------------------------------------------------ the checker
def _arena(nbytes=1000, fill=0x3C, guard_fill=0x5A):
    return M.Arena("buf", nbytes, "cpu", fill, guard_fill)


def test_arena_layout():
    for nbytes in (1, 1000, 4096 + 12):
        a = _arena(nbytes)
        assert a.payload.data_ptr() % 256 == 0 and a.payload.numel() == nbytes
        assert a.hi - a.lo == nbytes and a.lo >= M.GUARD and a.raw.numel() - a.hi >= M.GUARD
        assert bool((a.payload == 0x3C).all()) and bool((a.raw[:a.lo] == 0x5A).all()) and bool((a.raw[a.hi:] == 0x5A).all())
        assert a.check() == []
    v = _arena(3 * 5 * 4).view(torch.float32, (3, 5))
    assert v.shape == (3, 5) and v.data_ptr() % 256 == 0


def test_guard_flags_a_byte_on_either_side():
    a = _arena()
    a.raw[a.lo - 1] = 0
    assert a.check() == [dict(name="buf", side="before", distance=1, count=1)]
    a = _arena()
    a.raw[a.hi] = 0                                     # the first byte past the payload: no slack hides it
    assert a.check() == [dict(name="buf", side="after", distance=1, count=1)]
    a = _arena()
    a.raw[a.raw.numel() - 1] = 0                        # the far end of the trailing guard
    assert a.check() == [dict(name="buf", side="after", distance=a.raw.numel() - a.hi, count=1)]
    a = _arena()
    a.raw[0] = 0
    a.raw[a.lo - 7] = 1
    a.raw[a.hi + 3] = 2
    assert a.check() == [dict(name="buf", side="before", distance=7, count=2), dict(name="buf", side="after", distance=4, count=1)]
    assert "buf: 2 byte(s) changed before the payload, nearest 7" in M.describe_guards(a.check())


def test_guard_ignores_writes_inside_the_payload():
    a = _arena()
    a.payload[0] = 0
    a.payload[-1] = 0
    a.view(torch.float32, (250,))[:] = float("nan")
    assert a.check() == []


def test_arena_set_tracks_inputs_and_guards():
    s = M.ArenaSet("cpu", 0xFF, 0xFF)
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    xd = s.input("x", x)
    lens = s.input("lens", torch.tensor([3, 1], dtype=torch.int32))
    out = s.output("out", torch.float32, (2, 3))
    ws = s.scratch("ws", 512)
    assert torch.equal(xd, x) and lens.tolist() == [3, 1] and bool(torch.isnan(out).all()) and ws.numel() == 512
    assert s.check() == [] and s.changed_inputs() == []
    out[:] = 1.0
    ws[:] = 7
    assert s.check() == [] and s.changed_inputs() == []
    xd[2, 3] = 0.5
    assert s.changed_inputs() == ["x"]
    s.arenas["lens"].raw[s.arenas["lens"].hi] = 0       # one element past a 2-entry length array
    assert [(f["name"], f["side"], f["distance"]) for f in s.check()] == [("lens", "after", 1)]


def test_bits_equal_compares_nans():
    a = torch.tensor([1.0, float("nan"), -0.0])
    assert M.bits_equal(a, a.clone()) and not torch.equal(a, a.clone())
    assert not M.bits_equal(a, torch.tensor([1.0, float("nan"), 0.0]))
    h = torch.tensor([1.0, float("nan")], dtype=torch.float16)
    assert M.bits_equal(h, h.clone()) and not M.bits_equal(h, h.float())


def _odd_map(B=3, T=70):
    from quickvc_official_amd import lib as L
    entry, _ = load_case("odd")
    model, *_ = regenerate(entry)
    cfg = L.make_config(dict(model.model_config, operand_dtype="f16"))
    emu = E.load_emu_windows()
    import ctypes
    n_ws = int(L.load_library().qvc_workspace_bytes(ctypes.byref(cfg), B, T))
    return E.workspace_map(emu, cfg, B, T), n_ws


def test_gap_check_flags_one_byte_in_a_gap_of_the_odd_config():
    bufs, n_ws = _odd_map()
    gaps = M.gap_ranges(bufs, n_ws)
    assert gaps and gaps[-1][1] == n_ws                 # the tail behind `post`
    assert sum(hi - lo for lo, hi in gaps) + sum(b["bytes"] for b in bufs) == n_ws
    assert all(0 < hi - lo < 256 for lo, hi in gaps)    # nothing but alignment slack
    ws = torch.full((n_ws,), 0x3C, dtype=torch.uint8)
    assert M.check_gaps(ws, bufs, 0x3C) == []
    for b in bufs:                                      # every mapped byte may change
        ws[b["offset"]:b["offset"] + b["bytes"]] = 0
    assert M.check_gaps(ws, bufs, 0x3C) == []
    lo, hi = gaps[len(gaps) // 2]
    ws[hi - 1] = 0
    assert M.check_gaps(ws, bufs, 0x3C) == [(hi - 1, 1)]
    ws[n_ws - 1] = 0
    assert M.check_gaps(ws, bufs, 0x3C) == [(hi - 1, 1), (n_ws - 1, 1)]


# ------------------------------------------------------------------ the emulated path from the three fills
def _mini(ragged, inter=None):
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_inputs, make_synthetic_state_dict
    cfg = dict(q.MINI_MODEL_CONFIG) if inter is None else dict(q.MINI_MODEL_CONFIG, inter_channels=inter)
    model = q.SynthesizerTrn(641, 32, **cfg)
    sd = make_synthetic_state_dict(model, 1234)
    lens = [40, 17, 2] if ragged else None
    B, T = (3, 40) if ragged else (2, 24)
    unit, g, noise = make_synthetic_inputs(B, T, 256, cfg["inter_channels"], cfg["gin_channels"], seed0=40)
    if ragged:
        for b, n in enumerate(lens):
            unit[b, :, n:] = float("nan")               # "the padding's content is ignored"
            noise[b, :, n:] = float("nan")
    return model.model_config, sd, unit, g, noise, lens


@pytest.mark.parametrize("case", ["mini-ragged", "mini-plain", "mini-inter256"])
def test_emulated_path_is_independent_of_what_the_buffers_held(case):
    mc, sd, unit, g, noise, lens = _mini(case == "mini-ragged", 256 if case == "mini-inter256" else None)
    run = E.window_run(mc, sd, unit, g, noise, dtype="f16", lens=lens)
    N, kinds = run.steps()
    assert ("sample" in kinds) == (case == "mini-inter256"), kinds
    bufs = E.workspace_map(run.emu, run.cfg, run.B, run.T)
    outs = []
    for fill, _guard in M.FILLS:
        ws, out = run.run(0, N, E.junk_snapshot(run, fill))
        assert M.check_gaps(ws, bufs, fill) == [], (case, hex(fill))
        outs.append(out)
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    for fill, out in zip(M.FILLS[1:], outs[1:]):
        assert M.bits_equal(out, outs[0]), (case, hex(fill[0]))
    if lens is not None:
        spf = E.samples_per_frame(run.cfg)
        rows = outs[0].reshape(run.B, -1)
        for b, n in enumerate(lens):
            assert float(rows[b, n * spf:].abs().max() if n < run.T else 0.0) == 0.0, b
