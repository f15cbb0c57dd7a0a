"""CPU tests (no GPU) of the tick form of the windowed step (include/qvc.h: qvc_live_tick*; csrc/qvc_stream.h:
live_tick): per call, slot b brings n = clamp(n_new[b], 0, hop) frames.  The C ABI's surface, sizes and error codes on
the product library, and -- through the CPU twin of the driver (tools/emu_twin.cpp: live_tick on a backend derived from
the frozen emulation's, with the host version of the count-aware batched copy) -- the properties that define it:

  T1  the first n * spf samples of a tick's row are frames [pos - L, pos - L + n) of the OFFLINE conversion of the
      stream's first min(len, pos + n) frames, zeros outside [0, len); the rest of the row is 0.0; pos += n; a slot with
      n = 0 leaves no trace;
  T2  with L = C the concatenated output is the whole-utterance conversion however the stream was cut into ticks;
  T3  with every n = hop the outputs are bit for bit qvc_live_step's (the same twin).

The references are the emulation's own offline results and the comparison is bit equality (the SNR is printed first).
The twin covers the band-synthesis decoders and the pointer form of the noise only, as the emulation.
"""
import ctypes
import functools
import os
import re

import pytest
import torch

import config_space as CS
import tick_patterns as TP
from helpers import ROOT, snr_db
from live_common import NAN, _aligned, _context, _spf, built, twin_library  # noqa: F401

NEW = ("qvc_live_tick_state_bytes", "qvc_live_tick_workspace_bytes", "qvc_live_tick", "qvc_live_tick_rng", "qvc_live_tick_reset_slot")


@pytest.fixture(scope="module")
def twin(built):
    lib = twin_library()
    yield lib
    lib.qvc_emu_live_tick_trim(1)


@pytest.fixture(scope="module")
def lockstep(built):
    """The twin of qvc_live_step (T3's other side): the same library."""
    lib = twin_library()
    yield lib
    lib.qvc_emu_live_trim(1)


@functools.lru_cache(maxsize=None)
def _mini():
    """(model_config, state_dict) of MINI_MODEL_CONFIG with synthetic weights."""
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_state_dict
    model = q.SynthesizerTrn(641, 32, **q.MINI_MODEL_CONFIG)
    return model.model_config, make_synthetic_state_dict(model, 1234)


def _cfg_of(mc, dtype="f16"):
    from quickvc_official_amd import lib as L
    return L.make_config(dict(mc, operand_dtype=dtype))


# ---------------------------------------------------------------- surface
def test_exports_and_abi(built):
    header = open(os.path.join(ROOT, "include", "qvc.h")).read()
    for name in NEW:
        assert hasattr(built, name), name
        assert re.search(r"\b%s\(" % name, header), name
    assert built.qvc_abi_version() == 8 and "#define QVC_ABI_VERSION 8" in header


def test_frozen_emulation_lacks_the_tick_symbols(built):
    import emu
    from quickvc_official_amd import lib as L
    emulib = emu.load_emu()
    assert not hasattr(emulib, "qvc_emu_live_tick")
    L.declare(emulib, prefix="qvc_emu")


def test_sizes_are_positive_and_grow(built):
    import quickvc_official_amd as q
    from quickvc_official_amd import lib as L
    cfgs = {name: L.make_config(q.SynthesizerTrn(641, 32, **getattr(q, name)).model_config)
            for name in ("DEFAULT_MODEL_CONFIG", "MINI_MODEL_CONFIG", "ISTFT_MODEL_CONFIG")}
    cfgs["one_up8"] = L.make_config(CS.problem("one_up8")[1])
    for name, cfg in cfgs.items():
        p = ctypes.byref(cfg)
        C = _context(built, cfg)
        last = (0, 0)
        for hop, L_ in ((1, 0), (16, 0), (16, 8), (16, C), (320, C)):      # ordered: hop, then look_ahead, then hop
            s, w = int(built.qvc_live_tick_state_bytes(p, 4, hop, L_)), int(built.qvc_live_tick_workspace_bytes(p, 4, hop, L_))
            assert s > 0 and w > 0 and s % 256 == 0 and w % 256 == 0, (name, hop, L_, s, w)
            assert s > last[0] and w > last[1], (name, hop, L_)
            last = (s, w)
            assert w > int(built.qvc_workspace_bytes(p, 4, C + L_ + hop)), (name, hop, L_)
            assert w > int(built.qvc_live_workspace_bytes(p, 4, hop, L_)), (name, hop, L_)     # + the effective positions
        one, two = int(built.qvc_live_tick_state_bytes(p, 1, 16, 8)), int(built.qvc_live_tick_state_bytes(p, 2, 16, 8))
        assert one < two <= 2 * one
        w1, w2 = int(built.qvc_live_tick_workspace_bytes(p, 1, 16, 8)), int(built.qvc_live_tick_workspace_bytes(p, 2, 16, 8))
        assert w1 < w2


def test_error_codes(built):
    mc, _sd = _mini()
    cfg = _cfg_of(mc)
    p = ctypes.byref(cfg)
    C = _context(built, cfg)
    bad = CS.negative_config("n_flows_3")
    assert "n_flows_3" in CS.NEGATIVE
    for q in (built.qvc_live_tick_state_bytes, built.qvc_live_tick_workspace_bytes):
        assert q(p, 4, 0, 0) == -1 and q(p, 4, -3, 0) == -1               # hop < 1
        assert q(p, 0, 16, 0) == -1                                       # batch < 1
        assert q(p, 4, 16, -1) == -1 and q(p, 4, 16, C + 1) == -1         # look_ahead outside [0, C]
        assert q(p, 4, 16, C) > 0
        assert q(None, 4, 16, 0) == -1
        assert q(ctypes.byref(bad), 4, 16, 0) == -2
    n_state, n_ws = int(built.qvc_live_tick_state_bytes(p, 3, 7, 4)), int(built.qvc_live_tick_workspace_bytes(p, 3, 7, 4))
    a = 1 << 20                                                            # any 256-byte aligned non-null address
    # None of these calls gets as far as a launch: every pointer is checked (never followed) on the host first.
    from quickvc_official_amd import lib as L
    rng = L.QvcNoiseRng(5, a, 1.0)

    def tick(fn, draw, cfg_=cfg, blob=a, state=a, ns=n_state, unit=a, g=a, out=a, B=3, hop=7, L_=4, n_new=a, pos=a, ln=a, ws=a, nw=n_ws):
        return fn(ctypes.byref(cfg_), blob, state, ns, unit, g, draw, out, B, hop, L_, n_new, pos, ln, ws, nw, None)
    for fn, draw in ((built.qvc_live_tick, a), (built.qvc_live_tick_rng, ctypes.byref(rng))):
        assert tick(fn, draw, hop=0) == -1 and tick(fn, draw, hop=-2) == -1 and tick(fn, draw, B=0) == -1
        assert tick(fn, draw, L_=-1) == -1 and tick(fn, draw, L_=C + 1) == -1
        assert tick(fn, draw, cfg_=bad) == -2
        assert tick(fn, draw, ns=n_state - 1) == -5 and tick(fn, draw, nw=n_ws - 1) == -5      # before any launch
        for null in ("blob", "state", "unit", "g", "out", "n_new", "pos", "ln", "ws"):
            assert tick(fn, draw, **{null: None}) == -1, null
        assert tick(fn, None) == -1                                        # neither noise_new nor rng
        assert tick(fn, draw, ws=a + 4) == -1 and tick(fn, draw, state=a + 4) == -1
    no_keys = type(rng)(5, None, 1.0)
    assert tick(built.qvc_live_tick_rng, ctypes.byref(no_keys)) == -1
    reset = built.qvc_live_tick_reset_slot
    assert reset(p, a, n_state, 3, 7, 4, 3, 10, a, a, None) == -1 and reset(p, a, n_state, 3, 7, 4, -1, 10, a, a, None) == -1
    assert reset(p, a, n_state, 3, 7, 4, 1, -1, a, a, None) == -1 and reset(p, None, n_state, 3, 7, 4, 1, 10, a, a, None) == -1
    assert reset(p, a, n_state, 3, 0, 4, 1, 10, a, a, None) == -1 and reset(p, a, n_state, 3, 7, C + 1, 1, 10, a, a, None) == -1
    assert reset(ctypes.byref(bad), a, n_state, 3, 7, 4, 1, 10, a, a, None) == -2
    assert reset(p, a, n_state - 1, 3, 7, 4, 1, 10, a, a, None) == -5


# ---------------------------------------------------------------- the CPU twin
def _ring_ranges(twin, p, B, hop, L_):
    """[slot][which] -> (offset, bytes) of the slot's unit / noise ring in the state."""
    out = []
    for b in range(B):
        per = []
        for which in (0, 1):
            off, n = ctypes.c_int64(0), ctypes.c_int64(0)
            assert twin.qvc_emu_live_tick_ring(p, B, hop, L_, b, which, ctypes.byref(off), ctypes.byref(n)) == 0
            per.append((int(off.value), int(n.value)))
        out.append(per)
    return out


def _tick_stream(built, twin, mc, sd, unit, g, noise, lens, hop, L_, count_of, dtype="f16", trim=True):
    """Ticks `lens[b]` frames of every row through qvc_emu_live_tick with n_new[b] = count_of(b, tick, hop) until all have
    flushed.  State, workspace and the output chunk start from NaN bytes; every slot is started by the twin's reset;
    columns of unit_new / noise_new from n on, frames past a stream's end and the whole rows of idle slots are NaN.  After
    every tick: pos equals the sum of the clamped counts, and the ring bytes of a slot that was idle are what they were.
    -> [(positions before, clamped counts, chunk (B, hop * spf))] per tick."""
    from quickvc_official_amd import lib as L
    twin.qvc_emu_live_tick_trim(1 if trim else 0)
    cfg = _cfg_of(mc, dtype)
    p = ctypes.byref(cfg)
    blob = L.pack_weights(built, cfg, sd)
    B, UC, _T = unit.shape
    C_in = noise.shape[1]
    n_state, n_ws = int(built.qvc_live_tick_state_bytes(p, B, hop, L_)), int(built.qvc_live_tick_workspace_bytes(p, B, hop, L_))
    assert n_state > 0 and n_ws > 0
    _k1, state = _aligned(n_state, 0xFF)
    _k2, ws = _aligned(n_ws, 0xFF)
    pos = torch.full((B,), 12345, dtype=torch.int32)
    ln = torch.full((B,), -7, dtype=torch.int32)
    for b in range(B):
        assert twin.qvc_emu_live_tick_reset_slot(p, state.data_ptr(), n_state, B, hop, L_, b, int(lens[b]), pos.data_ptr(), ln.data_ptr()) == 0
    assert pos.tolist() == [0] * B and ln.tolist() == [int(v) for v in lens]
    rings = _ring_ranges(twin, p, B, hop, L_)
    g = g.float().contiguous()
    at = [0] * B
    ticks, k = [], 0
    while any(at[b] - L_ < lens[b] for b in range(B)):
        raw = [count_of(b, k, hop) for b in range(B)]
        n = [TP.clamp(v, hop) for v in raw]
        u_new, z_new = torch.full((B, UC, hop), NAN), torch.full((B, C_in, hop), NAN)
        for b, end in enumerate(lens):
            hi = min(at[b] + n[b], end)
            if hi > at[b]:
                u_new[b, :, :hi - at[b]] = unit[b, :, at[b]:hi]
                z_new[b, :, :hi - at[b]] = noise[b, :, at[b]:hi]
        counts = torch.tensor(raw, dtype=torch.int32)
        chunk = torch.full((B, hop * _spf(cfg)), NAN)
        before = [[state[o:o + m].clone() for o, m in rings[b]] for b in range(B)]
        st = twin.qvc_emu_live_tick(p, blob.data_ptr(), state.data_ptr(), n_state, u_new.data_ptr(), g.data_ptr(), z_new.data_ptr(),
                                    chunk.data_ptr(), B, hop, L_, counts.data_ptr(), pos.data_ptr(), ln.data_ptr(), ws.data_ptr(), n_ws)
        assert st == 0, st
        assert counts.tolist() == raw and ln.tolist() == [int(v) for v in lens]
        for b in range(B):
            if n[b] == 0:
                for (o, m), was in zip(rings[b], before[b]):
                    assert torch.equal(state[o:o + m], was), (k, b, "an idle slot's ring changed")
        ticks.append((list(at), n, chunk))
        at = [a + c for a, c in zip(at, n)]
        assert pos.tolist() == at, (k, pos.tolist(), at)
        k += 1
        assert k < 2000
    return ticks


def _check_ticks(ticks, want_of, lens, hop, L_, spf, what=""):
    """Every tick's chunk: samples from n * spf on are exactly 0; the first n * spf are frames [pos - L, pos - L + n) of
    want_of(b, prefix) (a 1-D waveform of the conversion of the stream's first `prefix` frames) -- bit-equal inside
    [0, len), exactly 0 outside.  -> the concatenated delivered waveform of every stream."""
    got = [torch.full((n * spf,), NAN) for n in lens]
    worst = float("inf")
    for at, n, chunk in ticks:
        for b, end in enumerate(lens):
            row = chunk[b]
            assert bool((row[n[b] * spf:] == 0).all()), (what, at, b, "not zero past n * spf")
            f0 = at[b] - L_
            lo, hi = max(f0, 0), min(f0 + n[b], end)
            inside = torch.zeros(hop * spf, dtype=torch.bool)
            if hi > lo:
                inside[(lo - f0) * spf:(hi - f0) * spf] = True
                ref = want_of(b, min(end, at[b] + n[b]))[lo * spf:hi * spf]
                have = row[inside]
                assert bool(torch.isfinite(have).all()), (what, at, b)
                worst = min(worst, snr_db(ref, have))
                assert torch.equal(have, ref), (what, at, b, n[b], snr_db(ref, have))
                got[b][lo * spf:hi * spf] = have
            assert bool((row[:n[b] * spf][~inside[:n[b] * spf]] == 0).all()), (what, at, b, "not zero outside the stream")
    print(f"{what}: worst delivered range {worst:.1f} dB against the offline prefix conversion")
    for b in range(len(lens)):
        assert bool(torch.isfinite(got[b]).all()), (what, b, "frames never delivered")
    return got


T_LENS, T_HOP, T_L = [23, 9], 4, 2


@functools.lru_cache(maxsize=None)
def _t_problem():
    from quickvc_official_amd.synth import make_synthetic_inputs
    mc, sd = _mini()
    unit, g, noise = make_synthetic_inputs(2, max(T_LENS), 256, mc["inter_channels"], mc["gin_channels"], seed0=8700)
    return mc, sd, unit, g, noise


@functools.lru_cache(maxsize=None)
def _t_prefix(b, prefix):
    """The emulated offline conversion of the first `prefix` frames of T stream b; computed once, read-only."""
    from emu import emu_infer_ragged
    mc, sd, unit, g, noise = _t_problem()
    t = max(prefix, 2)
    return emu_infer_ragged(mc, sd, unit[b:b + 1, :, :t].contiguous(), g[b:b + 1], noise[b:b + 1, :, :t].contiguous(), [prefix])[0, 0]


@pytest.mark.parametrize("trim", [True, False], ids=["trimmed", "plain"])
def test_twin_lockstep_is_a_special_case(built, twin, lockstep, trim):
    """T3, MINI_MODEL_CONFIG, streams of 23 and 9 frames, hop 4, L = 2: with every n = hop each tick's output is bit-equal
    to qvc_emu_live_step's on the same inputs."""
    from quickvc_official_amd import lib as L
    mc, sd, unit, g, noise = _t_problem()
    ticks = _tick_stream(built, twin, mc, sd, unit, g, noise, T_LENS, T_HOP, T_L, TP.all_hop, trim=trim)
    cfg = _cfg_of(mc)
    p = ctypes.byref(cfg)
    blob = L.pack_weights(built, cfg, sd)
    B = 2
    n_state, n_ws = int(built.qvc_live_state_bytes(p, B, T_HOP, T_L)), int(built.qvc_live_workspace_bytes(p, B, T_HOP, T_L))
    _k1, state = _aligned(n_state, 0xFF)
    _k2, ws = _aligned(n_ws, 0xFF)
    pos, ln = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    lockstep.qvc_emu_live_trim(1 if trim else 0)
    for b in range(B):
        assert lockstep.qvc_emu_live_reset_slot(p, state.data_ptr(), n_state, B, T_HOP, T_L, b, T_LENS[b], pos.data_ptr(), ln.data_ptr()) == 0
    gg = g.float().contiguous()
    assert len(ticks) == -(-(max(T_LENS) + T_L) // T_HOP)
    for k, (at, n, chunk) in enumerate(ticks):
        s = k * T_HOP
        assert at == [s] * B and n == [T_HOP] * B
        u_new, z_new = torch.full((B, 256, T_HOP), NAN), torch.full((B, noise.shape[1], T_HOP), NAN)
        for b, end in enumerate(T_LENS):
            hi = min(s + T_HOP, end)
            if hi > s:
                u_new[b, :, :hi - s] = unit[b, :, s:hi]
                z_new[b, :, :hi - s] = noise[b, :, s:hi]
        pos.fill_(s)
        want = torch.full_like(chunk, NAN)
        st = lockstep.qvc_emu_live_step(p, blob.data_ptr(), state.data_ptr(), n_state, u_new.data_ptr(), gg.data_ptr(), z_new.data_ptr(),
                                        want.data_ptr(), B, T_HOP, T_L, pos.data_ptr(), ln.data_ptr(), ws.data_ptr(), n_ws)
        assert st == 0
        assert bool(torch.isfinite(want).all()) and torch.equal(chunk, want), (k, "the tick with n = hop differs from the lockstep step")


@pytest.mark.parametrize("trim", [True, False], ids=["trimmed", "plain"])
def test_twin_prefix_exactness(built, twin, trim):
    """T1 on the same streams with the fixed pattern of tests/tick_patterns.py: n = 0 for slot 0 at the first tick, n = 1
    at pos 0, n = hop, each slot idle for three ticks while the other runs, -3 and hop + 5, the stream end inside a tick
    and flush ticks behind it."""
    mc, sd, unit, g, noise = _t_problem()
    seen = set()

    def count_of(b, k, hop):
        seen.add(TP.raw_count(b, k, hop))
        return TP.raw_count(b, k, hop)
    ticks = _tick_stream(built, twin, mc, sd, unit, g, noise, T_LENS, T_HOP, T_L, count_of, trim=trim)
    assert {-3, 0, 1, 2, 3, T_HOP, T_HOP + 5} <= seen
    assert ticks[0][1][0] == 0 and ticks[0][0][1] == 0 and ticks[0][1][1] == 1 and ticks[1][0][0] == 0 and ticks[1][1][0] == 1
    assert [t[1][1] for t in ticks[1:4]] == [0, 0, 0] and all(t[1][0] > 0 for t in ticks[1:4])
    assert [t[1][0] for t in ticks[7:10]] == [0, 0, 0] and all(t[1][1] > 0 for t in ticks[7:10])
    for b, end in enumerate(T_LENS):      # the end falls inside a tick, and ticks follow it
        assert any(at[b] < end < at[b] + n[b] for at, n, _c in ticks), b
        assert any(at[b] >= end and n[b] > 0 for at, n, _c in ticks), b
    mcfg = _cfg_of(mc)
    _check_ticks(ticks, _t_prefix, T_LENS, T_HOP, T_L, _spf(mcfg), "MINI hop 4 L 2")


def test_twin_chunking_invariance_at_full_look_ahead(built, twin):
    """T2 on row one_up8 (one up-sampler), f16, L = C, hop 5: one stream of W + 3 * hop + 1 frames cut into full ticks,
    into ticks of one frame and by the fixed mixed pattern.  Each cut is bit-equal to the whole-utterance emulation."""
    from emu import emu_infer_ragged
    from quickvc_official_amd.synth import make_synthetic_inputs
    _cfg, mc, sd = CS.problem("one_up8")
    cfg = _cfg_of(mc)
    C = _context(built, cfg)
    hop = 5
    W = 2 * C + hop
    T = W + 3 * hop + 1
    unit, g, noise = make_synthetic_inputs(1, T, 256, mc["inter_channels"], mc["gin_channels"], seed0=8800)
    whole = emu_infer_ragged(mc, sd, unit, g, noise, [T])[0, 0]
    spf = _spf(cfg)
    cuts = {}
    for name, count_of in (("full", TP.all_hop), ("ones", TP.all_one), ("mixed", TP.raw_count)):
        ticks = _tick_stream(built, twin, mc, sd, unit, g, noise, [T], hop, C, count_of)
        cuts[name] = _check_ticks(ticks, lambda b, prefix: whole, [T], hop, C, spf, f"one_up8 L = C = {C}, cut '{name}' ({len(ticks)} ticks)")[0]
        assert torch.equal(cuts[name], whole[:T * spf]), name
    assert torch.equal(cuts["full"], cuts["ones"]) and torch.equal(cuts["full"], cuts["mixed"])
