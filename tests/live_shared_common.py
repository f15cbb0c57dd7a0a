"""What tests/test_live_shared_host.py (the CPU twin) and tests/test_gpu_live_shared.py (the GPU) share: the two scenarios
that pin the SHARED rule of the window's rings (csrc/qvc_stream.h: live_rings) -- qvc_live_step and qvc_live_tick keep one
layout, the W - hop kept frames left-aligned, so they may alternate on one state -- written once over a small `calls`
object that hides where the buffers live:

    calls.device, calls.context                      where the tensors go; C of the window W = C + L + hop
    calls.sizes(B, hop, L, tick) -> (state, ws)      bytes, the tick's workspace with tick = True
    calls.buffer(n)                                  n bytes of 0xFF, 256-byte aligned
    calls.reset(state, B, hop, L, slot, length, pos, lens)
    calls.step(state, ws, unit_new, g, noise_new, out, pos, lens, L)            (pos is only read)
    calls.tick(state, ws, unit_new, g, noise_new, out, n_new, pos, lens, L)     (pos is advanced)
    calls.ring(B, hop, L, slot, which) -> (offset, bytes) of the slot's unit (0) / noise (1) ring in the state

MINI_MODEL_CONFIG, 2 slots of 30 and 26 frames, look-ahead 2.  NaN is fed wherever nothing may be read: columns from n on,
frames past a stream's end; such frames do reach the rings (masked by lens), in every run alike, so ring bytes are
compared as bytes.
"""
import ctypes
import random

import torch

import tick_patterns as TP

NAN = float("nan")
LENS, LOOK = [30, 26], 2


def mini_problem(seed0):
    """(model_config, state_dict, unit, g, noise) on the CPU."""
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_inputs, make_synthetic_state_dict
    model = q.SynthesizerTrn(641, 32, **q.MINI_MODEL_CONFIG)
    mc, sd = model.model_config, make_synthetic_state_dict(model, 1234)
    unit, g, noise = make_synthetic_inputs(len(LENS), max(LENS), 256, mc["inter_channels"], mc["gin_channels"], seed0=seed0)
    return mc, sd, unit.contiguous(), g.float().contiguous(), noise.contiguous()


def twin_ring(twin, cfg, B, hop, L, slot, which):
    off, n = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert twin.qvc_emu_live_tick_ring(ctypes.byref(cfg), B, hop, L, slot, which, ctypes.byref(off), ctypes.byref(n)) == 0
    return int(off.value), int(n.value)


def kept_bytes(calls, state, B, hop, L):
    """[slot] -> the kept W - hop frames of the slot's rings, as bytes on the CPU: (rows of both rings, (W - hop) * 4)."""
    W = calls.context + L + hop
    out = []
    for b in range(B):
        parts = []
        for which in (0, 1):
            off, n = calls.ring(B, hop, L, b, which)
            assert n % (W * 4) == 0
            parts.append(state[off:off + n].view(-1, W * 4)[:, :(W - hop) * 4])
        out.append(torch.cat(parts).cpu().clone())
    return out


def run(calls, unit, g, noise, hop, spf, kind_of, count_of=TP.all_hop):
    """Feeds LENS[b] frames of every slot until all have flushed: call k is calls.step when kind_of(k) == "step" (every slot
    hop frames; pos advanced here, as the caller of qvc_live_step does) and else calls.tick with n_new[b] = count_of(b, k, hop).
    noise None: the generator form.  One state, carved once with the tick's workspace size, started by calls.reset on 0xFF
    bytes.  -> [(kind, positions before, clamped counts, out on the CPU, kept_bytes after the call)]"""
    B, dev = len(LENS), calls.device
    n_state, n_ws = calls.sizes(B, hop, LOOK, True)
    assert n_state == calls.sizes(B, hop, LOOK, False)[0]
    state, ws = calls.buffer(n_state), calls.buffer(n_ws)
    pos, lens = torch.full((B,), 12345, dtype=torch.int32, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev)
    for b in range(B):
        calls.reset(state, B, hop, LOOK, b, LENS[b], pos, lens)
    assert pos.tolist() == [0] * B and lens.tolist() == LENS
    at, log, k = [0] * B, [], 0
    while any(at[b] - LOOK < LENS[b] for b in range(B)):
        kind = kind_of(k)
        raw = [hop] * B if kind == "step" else [count_of(b, k, hop) for b in range(B)]
        n = [TP.clamp(v, hop) for v in raw]
        u_new = torch.full((B, unit.shape[1], hop), NAN)
        z_new = None if noise is None else torch.full((B, noise.shape[1], hop), NAN)
        for b, end in enumerate(LENS):
            hi = min(at[b] + n[b], end)
            if hi > at[b]:
                u_new[b, :, :hi - at[b]] = unit[b, :, at[b]:hi]
                if z_new is not None:
                    z_new[b, :, :hi - at[b]] = noise[b, :, at[b]:hi]
        u_new, z_new = u_new.to(dev), None if z_new is None else z_new.to(dev)
        out = torch.full((B, hop * spf), NAN, device=dev)
        if kind == "step":
            calls.step(state, ws, u_new, g, z_new, out, pos, lens, LOOK)
            pos += hop
        else:
            calls.tick(state, ws, u_new, g, z_new, out, torch.tensor(raw, dtype=torch.int32, device=dev), pos, lens, LOOK)
        log.append((kind, list(at), n, out.cpu(), kept_bytes(calls, state, B, hop, LOOK)))
        at = [a + c for a, c in zip(at, n)]
        assert pos.tolist() == at and lens.tolist() == LENS, (k, kind)
        k += 1
        assert k < 400
    return log


def check_shared_state(calls, unit, g, noise, hop, spf, seed):
    """One state under a seeded mix of qvc_live_step and qvc_live_tick with every n = hop against the all-step run: every
    out torch.equal, and after every call the kept frames of each slot's rings equal, byte for byte."""
    rnd = random.Random(seed)
    kinds = [rnd.choice(["step", "tick"]) for _ in range(64)]
    kinds[:4] = ["tick", "step", "step", "tick"]                   # both hand-overs occur whatever the seed draws
    want = run(calls, unit, g, noise, hop, spf, lambda k: "step")
    got = run(calls, unit, g, noise, hop, spf, lambda k: kinds[k])
    assert len(got) == len(want) == -(-(max(LENS) + LOOK) // hop)
    used = [kind for kind, *_ in got]
    assert "step" in used[4:] and "tick" in used[4:], used
    for k, ((_kw, at_w, n_w, out_w, kept_w), (kind, at, n, out, kept)) in enumerate(zip(want, got)):
        assert at == at_w and n == n_w == [hop] * len(LENS)
        assert bool(torch.isfinite(out_w).all()) and torch.equal(out, out_w), (k, kind, "the mixed run's output differs from the all-step run's")
        for b in range(len(LENS)):
            assert torch.equal(kept[b], kept_w[b]), (k, kind, b, "the kept ring frames differ from the all-step run's")
    print(f"hop {hop}: {len(got)} calls, {used.count('tick')} of them ticks: outputs and kept ring bytes equal the all-step run's")


def check_state_after_ragged_ticks(calls, unit, g, noise, hop, spf):
    """The streams under the fixed pattern of tests/tick_patterns.py (idle ticks, n < hop) to the flush.  After every tick
    that moved a slot, the kept frames of its rings -- frames [pos - (W - hop), pos) -- equal, byte for byte, the same
    frames of a lockstep run that was fed the same frames: its kept frames at that pos where it passes through it (a
    multiple of hop), and otherwise the frames below q = pos - pos % hop of its state at q followed by the frames
    [q, pos) of its state at q + hop."""
    keep = calls.context + LOOK                                     # W - hop frames
    assert keep >= hop
    steps = run(calls, unit, g, noise, hop, spf, lambda k: "step")
    want = {(b, 0): torch.zeros_like(steps[0][4][b]) for b in range(len(LENS))}      # (slot, pos) -> kept bytes: a reset slot holds zeros
    for _kind, at, n, _out, kept in steps:
        for b in range(len(LENS)):
            want[(b, at[b] + n[b])] = kept[b]

    def lockstep_frames(b, p):
        q, d = p - p % hop, p % hop
        if d == 0 or (b, q + hop) not in want:
            return want.get((b, p))
        return torch.cat([want[(b, q)][:, d * 4:], want[(b, q + hop)][:, (keep - hop) * 4:(keep - hop + d) * 4]], dim=1)
    compared, ragged, aligned, counts = [0] * len(LENS), [0] * len(LENS), 0, set()
    for _kind, at, n, _out, kept in run(calls, unit, g, noise, hop, spf, lambda k: "tick", TP.raw_count):
        counts.update(n)
        for b in range(len(LENS)):
            ref = lockstep_frames(b, at[b] + n[b]) if n[b] > 0 else None
            if ref is None:                                         # idle, or past the last step of the lockstep run
                continue
            assert torch.equal(kept[b], ref), (b, at[b], n[b], "the kept ring frames differ from the lockstep run's")
            compared[b] += 1
            ragged[b] += 0 < n[b] < hop
            aligned += (at[b] + n[b]) % hop == 0
    assert {0, 1, 2, 3, hop} <= counts
    print(f"hop {hop}: ticks compared per slot {compared}, short ones {ragged}, at a pos of the lockstep run {aligned}")
    assert all(c >= 8 for c in compared) and all(r >= 4 for r in ragged) and aligned >= 1, (compared, ragged, aligned)
