"""CPU tests (no GPU) of the windowed streaming step with a bounded look-ahead (include/qvc.h: qvc_live_*;
csrc/qvc_stream.h: live_step): the C ABI's surface, sizes, error codes and the bound C on the receptive field, and --
through the CPU twin of the driver (tools/emu_twin.cpp: live_step on the frozen emulation's backend) -- the two
properties that define it:

  P1  a step's output is frames [pos - L, pos - L + hop) of the OFFLINE conversion of the stream's first
      min(len, pos + hop) frames;
  P2  with L = C the concatenated outputs are the whole-utterance conversion -- here for a decoder with one up-sampler,
      which qvc_stream_* refuses.

Both forms of the step run: trimmed (the default: rows a stage can no longer use are dropped before the next stage) and
plain (every stage over the whole window; the library's debug switch "live_trim" = 0).

Bar for both properties: >= 90 dB against the emulation's own offline result (the project's bar for streamed against offline;
measured: bit equality), and exact zeros outside the stream.  The twin covers the band-synthesis decoders and the
pointer form of the noise only: the emulation's backend is frozen before the single-band tail and the generator.
"""
import ctypes
import functools
import os
import re

import pytest
import torch

import config_space as CS
from helpers import ROOT, snr_db
from live_common import NAN, _aligned, _context, _spf, built, twin_library  # noqa: F401

NEW = ("qvc_live_context_frames", "qvc_live_state_bytes", "qvc_live_workspace_bytes", "qvc_live_step", "qvc_live_step_rng",
       "qvc_live_reset_slot")


@pytest.fixture(scope="module")
def twin(built):
    lib = twin_library()
    yield lib
    lib.qvc_emu_live_trim(1)


def _named_configs():
    """{name: qvc_config} of the three shipped model configs and three rows of the configuration space."""
    import quickvc_official_amd as q
    from quickvc_official_amd import lib as L
    out = {}
    for name in ("DEFAULT_MODEL_CONFIG", "MINI_MODEL_CONFIG", "ISTFT_MODEL_CONFIG"):
        out[name] = L.make_config(q.SynthesizerTrn(641, 32, **getattr(q, name)).model_config)
    for row in ("one_up8", "istft_ups3", "istft_ups4"):
        out[row] = L.make_config(CS.problem(row)[1])
    return out


def test_exports_and_abi(built):
    header = open(os.path.join(ROOT, "include", "qvc.h")).read()
    for name in NEW:
        assert hasattr(built, name), name
        assert re.search(r"\b%s\(" % name, header), name
    assert built.qvc_abi_version() == 8 and "#define QVC_ABI_VERSION 8" in header


def test_frozen_emulation_is_not_asked_for_the_new_symbols(built):
    import emu
    from quickvc_official_amd import lib as L
    emulib = emu.load_emu()
    assert not hasattr(emulib, "qvc_emu_live_step")
    L.declare(emulib, prefix="qvc_emu")


def test_sizes_are_positive_and_grow(built):
    for name, cfg in _named_configs().items():
        p = ctypes.byref(cfg)
        C = _context(built, cfg)
        assert C > 0, name
        last = (0, 0)
        for hop, L_ in ((1, 0), (16, 0), (16, 8), (16, C), (320, C)):      # ordered: hop, then look_ahead, then hop
            s, w = int(built.qvc_live_state_bytes(p, 4, hop, L_)), int(built.qvc_live_workspace_bytes(p, 4, hop, L_))
            assert s > 0 and w > 0 and s % 256 == 0 and w % 256 == 0, (name, hop, L_, s, w)
            assert s > last[0] and w > last[1], (name, hop, L_)
            last = (s, w)
            # the path's own workspace for the window is part of the step's
            assert w > int(built.qvc_workspace_bytes(p, 4, C + L_ + hop)), (name, hop, L_)
        one, two = int(built.qvc_live_state_bytes(p, 1, 16, 8)), int(built.qvc_live_state_bytes(p, 2, 16, 8))
        assert one < two <= 2 * one


def test_context_bounds(built):
    """84 <= C <= 90 on the shipped config (streaming.RECEPTIVE_FRAMES measured on the oracle; qvc_stream_lag_frames);
    C >= the left context measured on the emulation for two rows of the configuration space."""
    from quickvc_official_amd.streaming import RECEPTIVE_FRAMES
    cfgs = _named_configs()
    shipped = cfgs["DEFAULT_MODEL_CONFIG"]
    assert RECEPTIVE_FRAMES == 84
    assert 84 <= _context(built, shipped) <= 90 == int(built.qvc_stream_lag_frames(ctypes.byref(shipped)))
    from quickvc_official_amd import lib as L
    assert _context(built, L.make_config(CS.problem("wn_enc1_flow1")[1])) >= 25
    assert _context(built, cfgs["one_up8"]) >= 68


def test_error_codes(built):
    cfg = _named_configs()["MINI_MODEL_CONFIG"]
    p = ctypes.byref(cfg)
    C = _context(built, cfg)
    bad = CS.negative_config("n_flows_3")
    for q in (built.qvc_live_state_bytes, built.qvc_live_workspace_bytes):
        assert q(p, 4, 0, 0) == -1 and q(p, 4, -3, 0) == -1               # hop < 1
        assert q(p, 0, 16, 0) == -1                                       # batch < 1
        assert q(p, 4, 16, -1) == -1 and q(p, 4, 16, C + 1) == -1         # look_ahead outside [0, C]
        assert q(p, 4, 16, C) > 0
        assert q(None, 4, 16, 0) == -1
        assert q(ctypes.byref(bad), 4, 16, 0) == -2
    assert built.qvc_live_context_frames(None) == -1 and built.qvc_live_context_frames(ctypes.byref(bad)) == -2
    n_state, n_ws = int(built.qvc_live_state_bytes(p, 3, 7, 4)), int(built.qvc_live_workspace_bytes(p, 3, 7, 4))
    a = 1 << 20                                                            # any 256-byte aligned non-null address
    # None of these calls gets as far as a launch: every pointer is checked (never followed) on the host first.
    from quickvc_official_amd import lib as L
    rng = L.QvcNoiseRng(5, a, 1.0)

    def step(fn, draw, cfg_=cfg, blob=a, state=a, ns=n_state, unit=a, g=a, out=a, B=3, hop=7, L_=4, pos=a, ln=a, ws=a, nw=n_ws):
        return fn(ctypes.byref(cfg_), blob, state, ns, unit, g, draw, out, B, hop, L_, pos, ln, ws, nw, None)
    for fn, draw in ((built.qvc_live_step, a), (built.qvc_live_step_rng, ctypes.byref(rng))):
        assert step(fn, draw, hop=0) == -1 and step(fn, draw, B=0) == -1
        assert step(fn, draw, L_=-1) == -1 and step(fn, draw, L_=C + 1) == -1
        assert step(fn, draw, cfg_=bad) == -2
        assert step(fn, draw, ns=n_state - 1) == -5 and step(fn, draw, nw=n_ws - 1) == -5      # before any launch
        assert step(fn, draw, L_=5) == -5                                  # the buffers of a smaller window
        for null in ("blob", "state", "unit", "g", "out", "pos", "ln", "ws"):
            assert step(fn, draw, **{null: None}) == -1, null
        assert step(fn, None) == -1
        assert step(fn, draw, ws=a + 4) == -1 and step(fn, draw, state=a + 4) == -1
    no_keys = type(rng)(5, None, 1.0)
    assert step(built.qvc_live_step_rng, ctypes.byref(no_keys)) == -1
    reset = built.qvc_live_reset_slot
    assert reset(p, a, n_state, 3, 7, 4, 3, 10, a, a, None) == -1 and reset(p, a, n_state, 3, 7, 4, -1, 10, a, a, None) == -1
    assert reset(p, a, n_state, 3, 7, 4, 1, -1, a, a, None) == -1 and reset(p, None, n_state, 3, 7, 4, 1, 10, a, a, None) == -1
    assert reset(p, a, n_state, 3, 0, 4, 1, 10, a, a, None) == -1 and reset(p, a, n_state, 3, 7, C + 1, 1, 10, a, a, None) == -1
    assert reset(ctypes.byref(bad), a, n_state, 3, 7, 4, 1, 10, a, a, None) == -2
    assert reset(p, a, n_state - 1, 3, 7, 4, 1, 10, a, a, None) == -5


# ---------------------------------------------------------------- the CPU twin
def _twin_stream(built, twin, mc, sd, unit, g, noise, lens, hop, L_, dtype="f16", trim=True):
    """Streams `lens[b]` frames of every row through qvc_emu_live_step until all have flushed.  State, workspace and the
    output chunk start from NaN bytes; every slot is started by qvc_emu_live_reset_slot; the frames of unit_new /
    noise_new past a stream's end are NaN.  -> [(pos, chunk (B, hop * spf))] per step."""
    from quickvc_official_amd import lib as L
    twin.qvc_emu_live_trim(1 if trim else 0)
    cfg = L.make_config(dict(mc, operand_dtype=dtype))
    p = ctypes.byref(cfg)
    blob = L.pack_weights(built, cfg, sd)
    B, UC, _T = unit.shape
    C_in = noise.shape[1]
    n_state, n_ws = int(built.qvc_live_state_bytes(p, B, hop, L_)), int(built.qvc_live_workspace_bytes(p, B, hop, L_))
    assert n_state > 0 and n_ws > 0
    _k1, state = _aligned(n_state, 0xFF)
    _k2, ws = _aligned(n_ws, 0xFF)
    pos = torch.full((B,), 12345, dtype=torch.int32)
    ln = torch.full((B,), -7, dtype=torch.int32)
    for b in range(B):
        assert twin.qvc_emu_live_reset_slot(p, state.data_ptr(), n_state, B, hop, L_, b, int(lens[b]), pos.data_ptr(), ln.data_ptr()) == 0
    assert pos.tolist() == [0] * B and ln.tolist() == [int(v) for v in lens]
    g = g.float().contiguous()
    steps = []
    s = 0
    while s - L_ < max(lens):
        u_new, n_new = torch.full((B, UC, hop), NAN), torch.full((B, C_in, hop), NAN)
        for b, end in enumerate(lens):
            hi = min(s + hop, end)
            if hi > s:
                u_new[b, :, :hi - s] = unit[b, :, s:hi]
                n_new[b, :, :hi - s] = noise[b, :, s:hi]
        pos.fill_(s)
        chunk = torch.full((B, hop * _spf(cfg)), NAN)
        st = twin.qvc_emu_live_step(p, blob.data_ptr(), state.data_ptr(), n_state, u_new.data_ptr(), g.data_ptr(), n_new.data_ptr(),
                                    chunk.data_ptr(), B, hop, L_, pos.data_ptr(), ln.data_ptr(), ws.data_ptr(), n_ws)
        assert st == 0, st
        steps.append((s, chunk))
        s += hop
    return steps


def _check_against(steps, want_of_step, lens, hop, L_, spf):
    """Every step's chunk against want_of_step(pos) (B, 1, >= covered frames * spf): exact zeros outside [0, len), the
    frames inside concatenated per stream and compared at 90 dB."""
    B = len(lens)
    got = [torch.full((n * spf,), NAN) for n in lens]
    want = [torch.full((n * spf,), NAN) for n in lens]
    for s, chunk in steps:
        ref = want_of_step(s)
        f0 = s - L_
        for b, end in enumerate(lens):
            lo, hi = max(f0, 0), min(f0 + hop, end)
            inside = torch.zeros(hop * spf, dtype=torch.bool)
            if hi > lo:
                inside[(lo - f0) * spf:(hi - f0) * spf] = True
                got[b][lo * spf:hi * spf] = chunk[b, (lo - f0) * spf:(hi - f0) * spf]
                want[b][lo * spf:hi * spf] = ref[b, 0, lo * spf:hi * spf]
            outside = chunk[b][~inside]
            assert outside.numel() == 0 or bool((outside == 0).all()), (s, b, "not zero outside the stream")
    for b in range(B):
        assert bool(torch.isfinite(got[b]).all()) and bool(torch.isfinite(want[b]).all()), b
        db = snr_db(want[b], got[b])
        print(f"stream {b} ({lens[b]} frames): {db:.1f} dB")
        assert db >= 90.0, (b, db)


P1_LENS, P1_HOP = [97, 58, 7], 7


@functools.lru_cache(maxsize=None)
def _p1_prefix(s):
    """The emulated conversion of the prefixes the P1 streams have reached at position s; computed once, read-only."""
    from emu import emu_infer_ragged
    _cfg, mc, sd, unit, g, noise = _p1_problem()
    pre = [min(n, s + P1_HOP) for n in P1_LENS]
    t = max(pre)
    return emu_infer_ragged(mc, sd, unit[:, :, :t], g, noise[:, :, :t], pre)


@functools.lru_cache(maxsize=None)
def _p1_problem():
    from quickvc_official_amd.synth import make_synthetic_inputs
    _cfg, mc, sd = CS.problem("wn_enc1_flow1")
    unit, g, noise = make_synthetic_inputs(3, max(P1_LENS), 256, mc["inter_channels"], mc["gin_channels"], seed0=8100)
    return _cfg, mc, sd, unit, g, noise


@pytest.mark.parametrize("trim", [True, False], ids=["trimmed", "plain"])
@pytest.mark.parametrize("L_", [0, 4])
def test_twin_prefix_exactness(built, twin, L_, trim):
    """P1 on row wn_enc1_flow1 (WaveNet reach 10), f16: streams of 97, 58 and 7 frames at hop 7.  Every step is compared
    with emu_infer_ragged on the prefixes the streams have reached."""
    _cfg, mc, sd, unit, g, noise = _p1_problem()
    steps = _twin_stream(built, twin, mc, sd, unit, g, noise, P1_LENS, P1_HOP, L_, trim=trim)
    _check_against(steps, _p1_prefix, P1_LENS, P1_HOP, L_, CS.samples_per_frame(_cfg))


@pytest.mark.parametrize("trim", [True, False], ids=["trimmed", "plain"])
def test_twin_exact_streaming_one_upsampler(built, twin, trim):
    """P2 on row one_up8 (one up-sampler: qvc_stream_* refuses it), f16, L = C: the concatenated outputs of two streams
    of 45 and 17 frames at hop 20 equal the whole-utterance emulation."""
    from emu import emu_infer_ragged
    from quickvc_official_amd import lib as L
    from quickvc_official_amd.synth import make_synthetic_inputs
    _cfg, mc, sd = CS.problem("one_up8")
    cfg = L.make_config(dict(mc, operand_dtype="f16"))
    assert built.qvc_stream_state_bytes(ctypes.byref(cfg), 2, 20) == -2
    C = _context(built, cfg)
    lens, hop = [45, 17], 20
    unit, g, noise = make_synthetic_inputs(2, max(lens), 256, mc["inter_channels"], mc["gin_channels"], seed0=8200)
    steps = _twin_stream(built, twin, mc, sd, unit, g, noise, lens, hop, C, trim=trim)
    whole = emu_infer_ragged(mc, sd, unit, g, noise, lens)
    _check_against(steps, lambda s: whole, lens, hop, C, CS.samples_per_frame(_cfg))
