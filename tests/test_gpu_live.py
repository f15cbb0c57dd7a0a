"""The windowed streaming step with a bounded look-ahead on an MI355X (run with -m gpu): qvc_live_step / _rng /
_reset_slot through QvcEngine and streaming.LiveConverter.  GPU output is compared with GPU output of the offline path
(qvc_infer_batch_ragged[_rng]) at >= 90 dB, the bar of the other streaming tests (tests/test_gpu_parity.py:
test_incremental_streaming_*); frames outside a stream must be exact zeros.

  P1  a step's output is frames [pos - L, pos - L + hop) of the offline conversion of the stream's first
      min(len, pos + hop) frames (same g, same noise or the same (seed, key));
  P2  with L = C the concatenated outputs equal the whole-utterance conversion, for every decoder kind;
  P3  a stream's output does not depend on the other slots, on graph replay against direct launches, or on when its
      slot was admitted.

The step has two forms that must agree bit for bit: trimmed (the default: rows a stage can no longer use are dropped
before the next stage) and plain (every stage over the whole window; debug switch "live_trim" = 0).

The prefix conversions of one stream are rows of ONE ragged call: the stream's frames repeated once per step, the row
lengths the prefixes (generator form: rows with equal keys draw equal noise).
"""
import ctypes
import functools

import pytest
import torch

import config_space as CS
import memguard as M
from helpers import load_case, regenerate, snr_db
from live_common import NAN, SEED, _Model, _debug_switches_at_defaults, _keys, dev, lib, _prefix_rows, _row_model  # noqa: F401

pytestmark = pytest.mark.gpu

def _feed(conv, unit, noise, lens):
    """One step of every slot at the converter's positions: (positions before the step, chunk)."""
    S, hop = conv.streams, conv.hop
    u = torch.full((S, unit.shape[1], hop), NAN, device=unit.device)       # junk past the end must be ignored
    nz = None if noise is None else torch.full((S, noise.shape[1], hop), NAN, device=unit.device)
    pos = [conv.position(s) for s in range(S)]
    for s in range(S):
        a, b = pos[s], min(pos[s] + hop, lens[s])
        if b > a:
            u[s, :, :b - a] = unit[s, :, a:b]
            if nz is not None:
                nz[s, :, :b - a] = noise[s, :, a:b]
    return pos, conv.step(u, nz)


def _stream_all(conv, unit, g, noise, lens, keys=None, announce=True):
    """All slots started at once through start() (qvc_live_reset_slot) on a state full of NaN bytes; steps to the flush.
    -> [(positions, chunk)]"""
    conv._state.fill_(0xFF)
    for s in range(conv.streams):
        conv.start(s, g[s], length=lens[s] if announce else None, key=None if keys is None else keys[s])
    if not announce:
        conv.end(torch.tensor(lens, dtype=torch.int32))
    steps = []
    while not all(conv.finished(s) for s in range(conv.streams)):
        steps.append(_feed(conv, unit, noise, lens))
        assert len(steps) < 500
    return steps


def _check_steps(steps, slot, want_of_pos, n, hop, L, spf, what=""):
    """The chunks of one slot against want_of_pos(pos) (a 1-D waveform covering the delivered frames): zeros outside
    [0, n), the frames inside concatenated and compared at 90 dB."""
    got, want = torch.full((n * spf,), NAN), torch.full((n * spf,), NAN)
    for pos, chunk in steps:
        f0 = pos[slot] - L
        lo, hi = max(f0, 0), min(f0 + hop, n)
        c = chunk[slot].cpu()
        inside = torch.zeros(hop * spf, dtype=torch.bool)
        if hi > lo:
            inside[(lo - f0) * spf:(hi - f0) * spf] = True
            got[lo * spf:hi * spf] = c[inside]
            want[lo * spf:hi * spf] = want_of_pos(pos[slot])[lo * spf:hi * spf].cpu()
        assert bool((c[~inside] == 0).all()), (what, slot, pos[slot], "not zero outside the stream")
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(want).all()), (what, slot)
    db = snr_db(want, got)
    print(f"{what} slot {slot} ({n} frames): {db:.1f} dB")
    assert db >= 90.0, (what, slot, db)


# ---------------------------------------------------------------- P1
P1_LENS, P1_HOP = [97, 58, 7], 7


@functools.lru_cache(maxsize=None)
def _p1_problem():
    from quickvc_official_amd.synth import make_synthetic_inputs
    model, C = _row_model("wn_enc1_flow1")
    mc = model.model_config
    unit, g, noise = make_synthetic_inputs(3, max(P1_LENS), 256, mc["inter_channels"], mc["gin_channels"], seed0=8100)
    return model, C, unit.cuda(), g.cuda(), noise.cuda()


@functools.lru_cache(maxsize=None)
def _p1_reference(form):
    """{stream: {pos: waveform of the prefix the stream has reached at pos}} for every position a step can have;
    form = "rng" | "ptr".  Computed once, read-only."""
    model, _C, unit, g, noise = _p1_problem()
    out = {}
    for b, n in enumerate(P1_LENS):
        positions = list(range(0, max(P1_LENS) + 2 * P1_HOP, P1_HOP))
        prefixes = sorted({min(n, p + P1_HOP) for p in positions})
        rows = _prefix_rows(model.engine(), unit[b], g[b], None if form == "rng" else noise[b], _keys(3)[b], prefixes)
        out[b] = {p: rows[prefixes.index(min(n, p + P1_HOP)), 0] for p in positions}
    return out


@pytest.mark.parametrize("L", [0, 4])
def test_prefix_exactness_generator_form(lib, dev, L):
    """P1, row wn_enc1_flow1 (C = 35), streams of 97 / 58 / 7 frames at hop 7 (an odd hop: the 4-byte path of
    copy_batch), the noise from the generator; graph replay and direct launches give the same bits."""
    from quickvc_official_amd.streaming import LiveConverter
    model, C, unit, g, _noise = _p1_problem()
    ref = _p1_reference("rng")
    runs = []
    for graph in (True, False):
        conv = LiveConverter(model, 3, P1_HOP, L, use_graph=graph, seed=SEED)
        assert (conv._rng_graph is not None) == graph
        assert conv.lag == L and conv.noise_lag == 0 and conv.context == C == 35 and conv.window == C + L + P1_HOP
        runs.append(_stream_all(conv, unit, g, None, P1_LENS, keys=_keys(3)))
    for (_p, a), (_q, b) in zip(*runs):
        assert torch.equal(a, b)
    assert len(runs[0]) == len(runs[1]) == -(-(max(P1_LENS) + L) // P1_HOP)
    for b, n in enumerate(P1_LENS):
        _check_steps(runs[0], b, lambda p, b=b: ref[b][p], n, P1_HOP, L, model.samples_per_frame, f"rng L={L}")


def test_prefix_exactness_pointer_form(lib, dev):
    """P1 with the noise as a tensor per step, for the frames of unit_new (no noise lag); lengths written by end() after
    the slots were started.  The plain form of the step gives the bits of the trimmed one."""
    from quickvc_official_amd import lib as L
    from quickvc_official_amd.streaming import LiveConverter
    model, _C, unit, g, noise = _p1_problem()
    ref = _p1_reference("ptr")
    conv = LiveConverter(model, 3, P1_HOP, 4, use_graph=True)
    assert conv._graph is not None
    steps = _stream_all(conv, unit, g, noise, P1_LENS, announce=False)
    L.debug_set("live_trim", 0)                                           # read when the step is issued: a new capture
    plain = _stream_all(LiveConverter(model, 3, P1_HOP, 4, use_graph=True), unit, g, noise, P1_LENS, announce=False)
    L.debug_set("live_trim", 1)
    assert len(plain) == len(steps) and all(torch.equal(a, b) for (_p, a), (_q, b) in zip(steps, plain))
    for b, n in enumerate(P1_LENS):
        _check_steps(steps, b, lambda p, b=b: ref[b][p], n, P1_HOP, 4, model.samples_per_frame, "ptr L=4")


# ---------------------------------------------------------------- P2
@pytest.mark.parametrize("trim", [1, 0], ids=["trimmed", "plain"])
@pytest.mark.parametrize("name", ["one_up8", "mb_up16_up1", "istft_ups3", "istft_ups4", "rb_k1_k15_k13"])
def test_exact_streaming_for_every_decoder(lib, dev, name, trim):
    """P2: L = C, two streams of T = W + 3 * hop + 1 and T // 3 frames at hop 5 -- the window slides past the stream start
    and the short stream ends inside the first window.  One up-sampler, the multiband decoder with a stride-1 stage, the
    single-band decoder with three and four up-samplers (qvc_stream_* refuses all four), and the longest ResBlock halo.
    WaveNet (enc_layers, flow_layers, n_flows) = (2, 1, 2) keeps W small."""
    from quickvc_official_amd import lib as L
    from quickvc_official_amd.streaming import LiveConverter
    from quickvc_official_amd.synth import make_synthetic_inputs
    model, C = _row_model(name, wn=(2, 1, 2))
    mc, eng = model.model_config, model.engine()
    hop = 5
    L.debug_set("live_trim", trim)
    conv = LiveConverter(model, 2, hop, C, use_graph=True, seed=SEED)
    W = conv.window
    assert W == 2 * C + hop
    T = W + 3 * hop + 1
    lens = [T, T // 3]
    unit, g, _n = make_synthetic_inputs(2, T, 256, mc["inter_channels"], mc["gin_channels"], seed0=8300)
    unit, g = unit.cuda(), g.cuda()
    keys = _keys(2)
    whole = eng.infer_batch_ragged(unit, g, None, torch.tensor(lens, dtype=torch.int32), rng=(SEED, keys, 1.0)).clone()
    steps = _stream_all(conv, unit, g, None, lens, keys=keys)
    for b, n in enumerate(lens):
        _check_steps(steps, b, lambda p, b=b: whole[b, 0], n, hop, C, model.samples_per_frame, f"{name} C={C}")
    # ... and convert(), the convenience loop, gives the same
    streamed = conv.convert(unit, g, lengths=torch.tensor(lens, dtype=torch.int32), seed=SEED, keys=keys)
    assert snr_db(whole.cpu(), streamed.cpu()) >= 90.0
    assert float(streamed[1, :, lens[1] * model.samples_per_frame:].abs().max()) == 0.0


# ---------------------------------------------------------------- P3
def test_slots_admit_streams_independently(lib, dev):
    """P3: five streams through two slots at hop 6, L = 3, graph replay.  A stream is admitted when a slot is free (so
    slots sit at different positions and take over from a previous occupant), every other stream announces its length
    only when it ends (end_slot), and each is compared with ITS OWN prefix conversions: nothing of the other slot, of the
    previous occupant or of the admission step shows."""
    from quickvc_official_amd.streaming import LiveConverter
    from quickvc_official_amd.synth import make_synthetic_inputs
    model, _C = _row_model("wn_enc1_flow1")
    mc, eng, spf = model.model_config, model.engine(), model.samples_per_frame
    lens, S, hop, L = [40, 13, 29, 7, 22], 2, 6, 3
    N = len(lens)
    unit, g, _n = make_synthetic_inputs(N, max(lens), 256, mc["inter_channels"], mc["gin_channels"], seed0=8400)
    unit, g = unit.cuda(), g.cuda()
    keys = _keys(N)
    conv = LiveConverter(model, S, hop, L, use_graph=True, seed=SEED)
    conv.reset(lengths=torch.zeros(S, dtype=torch.int32))                  # every slot idle
    conv._state.fill_(0xFF)
    occupant, log = [None] * S, {i: [] for i in range(N)}
    nxt, done, n_steps, admitted_at = 0, 0, 0, {}
    while done < N:
        for s in range(S):
            if occupant[s] is None and nxt < N:
                conv.start(s, g[nxt], length=None if nxt % 2 else lens[nxt], key=keys[nxt])
                occupant[s], admitted_at[nxt] = nxt, n_steps
                nxt += 1
        u = torch.full((S, 256, hop), NAN, device=dev)
        pos = [conv.position(s) for s in range(S)]
        for s, i in enumerate(occupant):
            if i is None:
                continue
            a, b = pos[s], min(pos[s] + hop, lens[i])
            if b > a:
                u[s, :, :b - a] = unit[i, :, a:b]
            if i % 2 and pos[s] <= lens[i] < pos[s] + hop:
                conv.end_slot(s, lens[i])                                  # the stream ends inside this hop
        out = conv.step(u)
        n_steps += 1
        for s, i in enumerate(occupant):
            if i is None:
                continue
            log[i].append(([pos[s]], out[s:s + 1].clone()))
            if conv.finished(s):
                occupant[s], done = None, done + 1
        assert n_steps < 100
    assert len(set(admitted_at.values())) >= 3
    for i, n in enumerate(lens):
        positions = [p[0] for p, _c in log[i]]
        prefixes = sorted({min(n, p + hop) for p in positions})
        rows = _prefix_rows(eng, unit[i], g[i], None, keys[i], prefixes)
        _check_steps(log[i], 0, lambda p: rows[prefixes.index(min(n, p + hop)), 0], n, hop, L, spf, f"stream {i} admitted at step {admitted_at[i]}")


# ---------------------------------------------------------------- the stated size
def test_live_steps_at_stated_size(lib, dev):
    """The shipped config, 64 concurrent streams, hop 16, L = 8 (0.16 s behind the input instead of 1.8 s), `bf16x`, one
    graph replay per step, lengths unknown.  8 steps; steps 3 and 8 are checked against the prefix conversions of 8 of the
    streams."""
    import quickvc_official_amd as q
    from quickvc_official_amd.streaming import LiveConverter
    from quickvc_official_amd.synth import make_synthetic_inputs
    entry, _ = load_case("full_b1")
    _m, sd, _u, _g, _n = regenerate(entry)
    model = q.SynthesizerTrn(641, 32, **dict(entry["config"], operand_dtype="bf16x"))
    model.load_state_dict(sd)
    model = model.cuda().eval()
    S, hop, L, n_steps = 64, 16, 8, 8
    unit, g, noise = make_synthetic_inputs(S, hop * n_steps, 256, 192, 256, seed0=8500)
    unit, g, noise = unit.cuda(), g.cuda(), noise.cuda()
    conv = LiveConverter(model, S, hop, L, use_graph=True)
    assert conv._graph is not None and 84 <= conv.context <= 90 and conv.window == conv.context + L + hop
    conv.reset(g)
    eng, spf = model.engine(), model.samples_per_frame
    idx = list(range(0, S, 8))
    for k in range(1, n_steps + 1):
        p = (k - 1) * hop
        chunk = conv.step(unit[:, :, p:p + hop], noise[:, :, p:p + hop])
        assert chunk.shape == (S, hop * spf) and bool(torch.isfinite(chunk).all())
        if k in (3, 8):
            n = p + hop
            ref = eng.infer_batch_ragged(unit[idx, :, :n], g[idx], noise[idx, :, :n], torch.full((len(idx),), n, dtype=torch.int32))
            lo, hi = p - L, p - L + hop
            worst = min(snr_db(ref[j, 0, lo * spf:hi * spf].cpu(), chunk[i].cpu()) for j, i in enumerate(idx))
            print(f"step {k}: worst of {len(idx)} streams {worst:.1f} dB")
            assert worst >= 90.0, (k, worst)
    assert all(conv.position(s) == hop * n_steps for s in range(S))


# ---------------------------------------------------------------- memory contract
def _ptr(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("form", ["ptr", "rng"])
def test_memory_contract(lib, dev, form):
    """Every qvc_live_step[_rng] of three streams (23 / 9 / 16 frames, hop 7, L = 4, row wn_enc1_flow1) to the flush, raw C
    ABI, every caller-owned buffer in a guarded arena (tests/memguard.py) of exactly the queried size.  state, workspace,
    out, pos_dev and len_dev start from the fill (0x00 / 0x3C / 0xFF = NaN) and the slots are started by
    qvc_live_reset_slot; frames of unit_new / noise_new outside a stream are junk.  Guards intact, inputs unchanged, zeros
    outside the streams, outputs bit-equal across the fills and equal to LiveConverter's."""
    from quickvc_official_amd import lib as L
    from quickvc_official_amd.streaming import LiveConverter
    from quickvc_official_amd.synth import make_synthetic_inputs
    model, _C = _row_model("wn_enc1_flow1")
    mc, eng = model.model_config, model.engine()
    cfg = eng.cfg
    cfgp = ctypes.byref(cfg)
    lens, hop, L_ = [23, 9, 16], 7, 4
    S_, UC, C_in, spf = 3, 256, mc["inter_channels"], model.samples_per_frame
    unit, g, noise = make_synthetic_inputs(S_, max(lens), UC, C_in, mc["gin_channels"], seed0=8600)
    n_state, n_ws = int(lib.qvc_live_state_bytes(cfgp, S_, hop, L_)), int(lib.qvc_live_workspace_bytes(cfgp, S_, hop, L_))
    assert n_state > 0 and n_ws > 0
    keys = torch.tensor([k - (1 << 64) if k >> 63 else k for k in _keys(S_)], dtype=torch.int64)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    n_steps = -(-(max(lens) + L_) // hop)
    results = []
    for fill, guard in M.FILLS:
        A = M.ArenaSet(dev, fill, guard)
        junk = NAN if fill == 0xFF else 123.0
        bl, gg = A.input("blob", eng.blob.cpu()), A.input("g", g)
        kd = A.input("keys_dev", keys)
        state, ws = A.scratch("state", n_state), A.scratch("workspace", n_ws)
        out = A.output("out", torch.float32, (S_, hop * spf))
        pos, ln = A.output("pos_dev", torch.int32, (S_,)), A.output("len_dev", torch.int32, (S_,))
        for b, n in enumerate(lens):
            assert lib.qvc_live_reset_slot(cfgp, _ptr(state), n_state, S_, hop, L_, b, n, _ptr(pos), _ptr(ln), stream()) == 0
        torch.cuda.synchronize()
        assert pos.tolist() == [0] * S_ and ln.tolist() == lens
        rng = L.QvcNoiseRng(SEED, _ptr(kd), 1.0)
        whole = torch.zeros(S_, max(lens) * spf, device=dev)
        for k in range(n_steps):
            s = k * hop
            u_new, n_new = torch.full((S_, UC, hop), junk), torch.full((S_, C_in, hop), junk)
            for b, end in enumerate(lens):
                hi = min(s + hop, end)
                if hi > s:
                    u_new[b, :, :hi - s] = unit[b, :, s:hi]
                    n_new[b, :, :hi - s] = noise[b, :, s:hi]
            ud, nd = A.input("unit_new", u_new), A.input("noise_new", n_new)
            pos.fill_(s)
            out.view(torch.uint8).fill_(fill)
            if form == "ptr":
                st = lib.qvc_live_step(cfgp, _ptr(bl), _ptr(state), n_state, _ptr(ud), _ptr(gg), _ptr(nd), _ptr(out), S_, hop, L_,
                                       _ptr(pos), _ptr(ln), _ptr(ws), n_ws, stream())
            else:
                st = lib.qvc_live_step_rng(cfgp, _ptr(bl), _ptr(state), n_state, _ptr(ud), _ptr(gg), ctypes.byref(rng), _ptr(out), S_, hop, L_,
                                           _ptr(pos), _ptr(ln), _ptr(ws), n_ws, stream())
            torch.cuda.synchronize()
            assert st == 0, (hex(fill), k, st)
            assert A.changed_inputs() == [], (hex(fill), k)
            assert pos.tolist() == [s] * S_ and ln.tolist() == lens
            f0 = s - L_
            for b, end in enumerate(lens):
                lo, hi = max(f0, 0), min(f0 + hop, end)
                inside = torch.zeros(hop * spf, dtype=torch.bool, device=dev)
                if hi > lo:
                    inside[(lo - f0) * spf:(hi - f0) * spf] = True
                    whole[b, lo * spf:hi * spf] = out[b][inside]
                assert bool((out[b][~inside] == 0).all()), (hex(fill), k, b)
        damaged = A.check()
        assert not damaged, f"fill {fill:#x}: {M.describe_guards(damaged)}"
        assert bool(torch.isfinite(whole).all()), hex(fill)
        results.append(whole.clone())
    for (fill, _g), res in zip(M.FILLS[1:], results[1:]):
        assert M.bits_equal(res, results[0]), f"the output depends on what the buffers held: fill {fill:#x} differs from fill 0x0"
    conv = LiveConverter(model, S_, hop, L_, use_graph=False, seed=SEED if form == "rng" else None)
    steps = _stream_all(conv, unit.to(dev), g.to(dev), None if form == "rng" else noise.to(dev), lens, keys=_keys(S_))
    assert len(steps) == n_steps
    want = torch.zeros_like(results[0])
    for p, chunk in steps:
        for b, end in enumerate(lens):
            f0 = p[b] - L_
            lo, hi = max(f0, 0), min(f0 + hop, end)
            if hi > lo:
                want[b, lo * spf:hi * spf] = chunk[b, (lo - f0) * spf:(hi - f0) * spf]
    assert torch.equal(results[0], want), "the raw ABI run differs from LiveConverter's"
