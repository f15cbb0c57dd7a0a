"""CPU tests (no GPU) of the tick form of the segment rings (include/qvc.h: qvc_stream_tick*; csrc/qvc_stream.h:
stream_tick): per call, slot b brings n = clamp(n_new[b], 0, hop) frames, on qvc_stream_step's state.  The C ABI's surface
and status codes on the product library and, through the CPU twin of the driver (tools/emu_twin.cpp: stream_tick on a
backend derived from the frozen emulation's, with the host version of the count-aware batched copy):

  S1  with every n = hop, out and the ring bytes a later call can read are bit for bit qvc_stream_step's; the two calls
      alternate on one state;
  S2  under the fixed pattern of tests/tick_patterns.py a stream's concatenated output is its whole-utterance conversion
      (the emulation's own offline result, >= 90 dB; bit equality is printed), zeros where the contract says so;
  S3  the output does not depend on how the stream was cut into ticks;
  S4  columns [n, hop) of unit_new / noise_new are never read;
  S5  an idle slot leaves no trace (checked at every tick of every run: stream_tick_common.run_streams);
  S6  a slot's outputs do not depend on what its neighbours do.

Shapes: rows up16_k17_up2_k2 and mb_up16_up1 with the WaveNet (2, 1, 2), 3 slots, hops 4 and 5, streams of 37 / 23 / 9
frames.  The twin covers the pointer form of the noise only, as the emulation.
"""
import ctypes
import functools
import os
import re

import pytest
import torch

import config_space as CS
import stream_tick_common as SC
import tick_patterns as TP
from helpers import ROOT
from live_common import built, twin_library  # noqa: F401
from stream_tick_common import HOPS, LENS, ROW, ROW_MB

NEW = ("qvc_stream_tick_workspace_bytes", "qvc_stream_tick", "qvc_stream_tick_rng")


@pytest.fixture(scope="module")
def twin(built):
    return SC.declare_twin(twin_library())


@functools.lru_cache(maxsize=None)
def _whole(name):
    """The emulated whole-utterance conversion of the row's three streams; computed once, read-only."""
    from emu import emu_infer_ragged
    mc, sd = SC.row_problem(name)
    unit, g, noise = SC.row_inputs(name)
    return emu_infer_ragged(mc, sd, unit, g, noise, LENS)


def _runner(built, twin, name, hop, **kw):
    mc, sd = SC.row_problem(name)
    _unit, g, _noise = SC.row_inputs(name)
    return SC.TwinRunner(built, twin, mc, sd, g, len(LENS), hop, **kw)


@functools.lru_cache(maxsize=None)
def _cut(name, hop, which):
    """The ticks of the row's streams cut by `which`; computed once per (row, hop, cut), read-only."""
    from quickvc_official_amd import lib as L
    built, twin = L.load_library(), SC.declare_twin(twin_library())      # (built by the fixtures of the test that asks)
    unit, _g, noise = SC.row_inputs(name)
    R = _runner(built, twin, name, hop)
    seen = set()

    def count_of(b, k, h):
        v = {"pattern": TP.raw_count, "ones": TP.all_one, "full": TP.all_hop}[which](b, k, h)
        seen.add(v)
        return v
    ticks = SC.run_streams(R, unit, noise, LENS, count_of)
    return R, ticks, seen


# ---------------------------------------------------------------- surface
def test_exports_and_abi(built, twin):
    header = open(os.path.join(ROOT, "include", "qvc.h")).read()
    for name in NEW:
        assert hasattr(built, name), name
        assert re.search(r"\b%s\(" % name, header), name
    assert built.qvc_abi_version() == 8 and "#define QVC_ABI_VERSION 8" in header
    assert "keep lockstep" not in header
    assert hasattr(twin, "qvc_emu_stream_tick")


def test_a_backend_without_the_hook_gets_bad_config(built, twin):
    """The frozen emulation's backend does not state kStreamTick: the same driver answers QVC_ERR_BAD_CONFIG."""
    from quickvc_official_amd import lib as L
    import emu
    mc, _sd = SC.row_problem(ROW)
    cfg = L.make_config(mc)
    assert twin.qvc_emu_stream_tick_frozen(ctypes.byref(cfg), 3, 4) == -2
    assert not hasattr(emu.load_emu(), "qvc_emu_stream_tick")


def test_status_codes(built):
    import quickvc_official_amd as q
    from quickvc_official_amd import lib as L
    mc, _sd = SC.row_problem(ROW)
    cfg = L.make_config(mc)
    p = ctypes.byref(cfg)
    single = L.make_config(q.SynthesizerTrn(641, 32, **q.ISTFT_MODEL_CONFIG).model_config)
    one_up = L.make_config(CS.problem("one_up8")[1])
    assert int(single.n_ups) == 2 and int(one_up.n_ups) == 1
    size = built.qvc_stream_tick_workspace_bytes
    assert size(p, 3, 0) == -1 and size(p, 3, -2) == -1 and size(p, 0, 4) == -1 and size(None, 3, 4) == -1
    assert size(ctypes.byref(single), 3, 4) == -2 and size(ctypes.byref(one_up), 3, 4) == -2
    n_state, n_ws = int(built.qvc_stream_state_bytes(p, 3, 5)), int(size(p, 3, 5))
    assert n_state > 0 and n_ws > int(built.qvc_stream_workspace_bytes(p, 3, 5)) and n_ws % 256 == 0
    a = 1 << 20                                                            # any 256-byte aligned non-null address
    rng = L.QvcNoiseRng(5, a, 1.0)
    # None of these calls gets as far as a launch: every pointer is checked (never followed) on the host first.

    def tick(fn, draw, cfg_=cfg, blob=a, state=a, ns=n_state, unit=a, g=a, out=a, B=3, hop=5, n_new=a, pos=a, ln=a, ws=a, nw=n_ws):
        return fn(ctypes.byref(cfg_), blob, state, ns, unit, g, draw, out, B, hop, n_new, pos, ln, ws, nw, None)

    def step(fn, draw, **kw):            # qvc_stream_step with the same arguments: the codes must agree
        kw = dict(dict(cfg_=cfg, blob=a, state=a, ns=n_state, unit=a, g=a, out=a, B=3, hop=5, pos=a, ln=a, ws=a, nw=n_ws), **kw)
        return fn(ctypes.byref(kw["cfg_"]), kw["blob"], kw["state"], kw["ns"], kw["unit"], kw["g"], draw, kw["out"], kw["B"], kw["hop"],
                  kw["pos"], kw["ln"], kw["ws"], kw["nw"], None)
    for fn, sfn, draw in ((built.qvc_stream_tick, built.qvc_stream_step, a), (built.qvc_stream_tick_rng, built.qvc_stream_step_rng, ctypes.byref(rng))):
        assert tick(fn, draw, n_new=None) == -1
        assert tick(fn, draw, hop=0) == -1 and tick(fn, draw, hop=-2) == -1 and tick(fn, draw, B=0) == -1
        assert tick(fn, draw, ns=n_state - 1) == -5 and tick(fn, draw, nw=n_ws - 1) == -5
        assert tick(fn, draw, cfg_=single) == -2 and tick(fn, draw, cfg_=one_up) == -2
        assert tick(fn, None) == -1                                        # neither noise_new nor rng
        assert tick(fn, draw, ws=a + 4) == -1 and tick(fn, draw, state=a + 4) == -1
        for null in ("blob", "state", "unit", "g", "out", "pos", "ln", "ws"):
            assert tick(fn, draw, **{null: None}) == step(sfn, draw, **{null: None}) == -1, null
        # the order of the checks is the step's: a bad argument in front of a bad config in front of a short buffer
        for kw in (dict(B=0, cfg_=single), dict(cfg_=single, ns=1), dict(hop=0, ns=1), dict(unit=None, ns=1), dict(ns=1, nw=1)):
            assert tick(fn, draw, **kw) == step(sfn, draw, **kw), kw
    assert tick(built.qvc_stream_tick_rng, ctypes.byref(type(rng)(5, None, 1.0))) == -1


# ---------------------------------------------------------------- S1
@pytest.mark.parametrize("name,hop", [(ROW, 4), (ROW, 5), (ROW_MB, 5)])
def test_lockstep_is_the_special_case(built, twin, name, hop):
    """S1: after EVERY call out is torch.equal to qvc_stream_step's and so is the kept part of every row of every ring of
    every slot; a third state on which the two calls alternate gives the same outputs."""
    unit, _g, noise = SC.row_inputs(name)
    step_R, tick_R, mixed_R = (_runner(built, twin, name, hop) for _ in range(3))
    outs = {}
    for key, R, call in (("step", step_R, lambda k: "step"), ("tick", tick_R, None), ("mixed", mixed_R, lambda k: "step" if k % 2 else "tick")):
        states = []
        ticks = SC.run_streams(R, unit, noise, LENS, TP.all_hop, call=call,
                               between=lambda k, R_, at: (states.append(R_.state()) if k else None) or at)
        states.append(R.state())
        outs[key] = (ticks, states)
    (st_t, st_s), (tk_t, tk_s), (mx_t, _mx_s) = outs["step"], outs["tick"], outs["mixed"]
    assert len(st_t) == len(tk_t) == len(mx_t) == -(-(max(LENS) + step_R.lag) // hop)
    for k in range(len(st_t)):
        assert bool(torch.isfinite(st_t[k][2]).all())
        assert torch.equal(tk_t[k][2], st_t[k][2]), (k, "the tick with n = hop differs from the lockstep step")
        assert torch.equal(mx_t[k][2], st_t[k][2]), (k, "alternating step and tick on one state differs from lockstep alone")
        for b in range(len(LENS)):
            assert torch.equal(SC.kept_bytes(tk_s[k], tick_R.table, b), SC.kept_bytes(st_s[k], step_R.table, b)), (k, b, "ring bytes differ")


def test_launches_of_one_tick(built, twin):
    """A tick issues a step's number of data-movement launches, all of them copy_counted: 5 + n_flows."""
    name, hop = ROW, 4
    unit, _g, noise = SC.row_inputs(name)
    R = _runner(built, twin, name, hop)
    for b, n in enumerate(LENS):
        R.reset_slot(b, n)
    twin.qvc_emu_twin_counts(None)
    twin.qvc_emu_stream_tick_counts(None)
    u, z = SC.tick_inputs(unit, noise, [0, 0, 0], [1, 0, hop], LENS, hop, R.nlag)
    R.tick(u, z, [1, 0, hop])
    old, new = (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 2)()
    twin.qvc_emu_twin_counts(old)
    twin.qvc_emu_stream_tick_counts(new)
    nf = SC.WN[2]
    rings = len(R.table[0])
    assert rings == 1 + nf + 1 + 3
    # append + noise (3), 3 per coupling layer, the decoder's ring, 3 stage-0 rings, delivery + rings out, rings back
    assert list(old) == [0, 0, 0, 0] and list(new) == [5 + nf, 3 + 3 * nf + 1 + 3 + 1 + 2 * rings]


# ---------------------------------------------------------------- S2
@pytest.mark.parametrize("name,hop", [(ROW, 4), (ROW, 5), (ROW_MB, 4)])
def test_exactness_under_the_pattern(built, twin, name, hop):
    R, ticks, seen = _cut(name, hop, "pattern")
    SC.check_pattern_holds(ticks, LENS, hop, seen)
    whole = _whole(name)
    for b, length in enumerate(LENS):
        got = SC.collect(ticks, b, length, R.lag, R.spf, f"{name} hop {hop}")
        SC.compare(whole[b, 0, :length * R.spf], got, f"{name} hop {hop} slot {b} ({length} frames, {len(ticks)} ticks) against the whole utterance")


# ---------------------------------------------------------------- S3
@pytest.mark.parametrize("hop", HOPS)
def test_independence_of_the_cut(built, twin, hop):
    cuts = {}
    for which in ("pattern", "ones", "full"):
        R, ticks, _seen = _cut(ROW, hop, which)
        cuts[which] = [SC.collect(ticks, b, length, R.lag, R.spf, which) for b, length in enumerate(LENS)]
    for x, y in (("pattern", "ones"), ("pattern", "full"), ("ones", "full")):
        for b in range(len(LENS)):
            SC.compare(cuts[x][b], cuts[y][b], f"hop {hop} slot {b}: cut '{x}' against cut '{y}'")


# ---------------------------------------------------------------- S4
@pytest.mark.parametrize("hop", HOPS)
def test_unused_columns_are_never_read(built, twin, hop):
    """The pattern's run feeds NaN in columns [n, hop), in the whole rows of idle slots and past a stream's end; the same
    run with 0.25 there is torch.equal, and finite."""
    unit, _g, noise = SC.row_inputs(ROW)
    _R, nan_ticks, _seen = _cut(ROW, hop, "pattern")
    R = _runner(built, twin, ROW, hop)
    clean = SC.run_streams(R, unit, noise, LENS, TP.raw_count, junk=0.25)
    assert len(clean) == len(nan_ticks)
    for (a0, n0, o0), (a1, n1, o1) in zip(nan_ticks, clean):
        assert a0 == a1 and n0 == n1 and bool(torch.isfinite(o0).all()) and torch.equal(o0, o1), a0


# ---------------------------------------------------------------- S5 / S6
def test_idle_ticks_occur_and_leave_no_trace(built, twin):
    """S5 is asserted inside run_streams at every tick; here: the pattern's runs did hold idle ticks of every slot, at
    pos 0 and mid-stream, and the idle rows of `out` are zeros."""
    _R, ticks, _seen = _cut(ROW, 5, "pattern")
    for b in range(len(LENS)):
        idle = [(at[b], out[b]) for at, n, out in ticks if n[b] == 0]
        assert len(idle) >= 3 and any(a > 0 for a, _o in idle), b
        assert all(bool((o == 0).all()) for _a, o in idle)
    assert ticks[0][1][0] == 0 and ticks[0][0][0] == 0


@pytest.mark.parametrize("hop", HOPS)
def test_slots_tick_independently(built, twin, hop):
    """S6: slot 1's outputs, tick by tick, with its neighbours ticking by the pattern, idle throughout, and re-admitted
    with qvc_stream_reset_slot mid-stream (slot 0 at tick 5, slot 2 at ticks 3 and 9)."""
    unit, _g, noise = SC.row_inputs(ROW)
    _R, base, _seen = _cut(ROW, hop, "pattern")

    def alone(b, k, h):
        return TP.raw_count(b, k, h) if b == 1 else 0

    def readmit(k, R, at):
        at = list(at)
        for slot, when in ((0, (5,)), (2, (3, 9))):
            if k in when:
                R.reset_slot(slot, LENS[slot])
                at[slot] = 0
        return at
    runs = [SC.run_streams(_runner(built, twin, ROW, hop), unit, noise, LENS, alone, watch=[1]),
            SC.run_streams(_runner(built, twin, ROW, hop), unit, noise, LENS, TP.raw_count, watch=[1], between=readmit)]
    for ticks in runs:
        assert len(ticks) <= len(base)
        for (a0, n0, o0), (a1, n1, o1) in zip(base, ticks):
            assert a0[1] == a1[1] and n0[1] == n1[1] and torch.equal(o0[1], o1[1]), (hop, a0)
