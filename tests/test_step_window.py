"""Step windows of the launch sequence, on the host emulation (no GPU needed).

Path<> counts every backend call that enqueues device work as one step and issues only the steps inside its window
(csrc/qvc_path.h).  The GPU step test (test_gpu_step_parity.py) stops the product after step n, copies the workspace
and the output to the host, and replays step n on the emulation from that copy.  That is sound only if the path keeps
no state outside those two buffers: checked here as "steps [0, n) then [n, end) from the snapshot == one run", bit
for bit, at every split point.  The comparator the GPU test uses is checked here too: it must flag a kernel that is
slightly wrong in one place and stay quiet about realistic rounding noise and about rows past a ragged member's end.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

import emu as E
import stepcheck as S
from helpers import load_case, regenerate


def _run(name, dtype, ragged, switches=None, T=None, B=None):
    entry, _ = load_case(name)
    if T is not None or B is not None:
        entry = dict(entry, frames=T or entry["frames"], batch=B or entry["batch"])
    model, sd, unit, g, noise = regenerate(entry)
    B, _, T = unit.shape
    lens = None
    if ragged:
        lens = [T - 3, 2] + [T] * (B - 2)
        unit, noise = unit.clone(), noise.clone()
        for b, n in enumerate(lens):
            unit[b, :, n:] = 300.0 * (b + 1)           # junk the path must never read unmasked
            noise[b, :, n:] = -55.0
    return E.window_run(model.model_config, sd, unit, g, noise, dtype=dtype, lens=lens, switches=switches)


def _run_shipped(switches, B=1, T=140):
    """The shipped config (synthetic weights): the only one whose k 3 ResBlocks the chained kernel takes, and only past
    the few-tiles batch size (B * frames * 20 * 3 chains > 8192 at stage 1)."""
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_state_dict, make_synthetic_inputs
    model = q.SynthesizerTrn(641, 32, **q.DEFAULT_MODEL_CONFIG)
    sd = make_synthetic_state_dict(model, 17)
    unit, g, noise = make_synthetic_inputs(B, T, 256, 192, 256, seed0=17)
    return E.window_run(model.model_config, sd, unit, g, noise, switches=switches)


def _decomposes(run):
    """[0, n) then [n, N) from the snapshot == [0, N), bit for bit, for every n; returns the step kinds."""
    N, kinds = run.steps()
    assert N == len(kinds) and N > 0
    s0 = E.junk_snapshot(run)
    whole = run.run(0, N, s0)
    assert not torch.equal(whole[0], s0[0])
    def split(n):                                  # ctypes releases the GIL: the splits run in parallel
        rest = run.run(n, N, run.run(0, n, s0))
        return torch.equal(rest[0], whole[0]), torch.equal(rest[1], whole[1])
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        same = list(ex.map(split, range(N + 1)))
    for n, (ws_same, out_same) in enumerate(same):
        assert ws_same, f"workspace differs after the split at step {n} ({kinds[n] if n < N else 'end'})"
        assert out_same, f"output differs after the split at step {n}"
    # a window past the end, or an empty one, issues nothing
    assert torch.equal(run.run(N, N + 5, whole)[0], whole[0])
    return kinds


@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "ragged"])
@pytest.mark.parametrize("dtype", ["f16", "bf16x"])
@pytest.mark.parametrize("name", ["mini", "odd", "mini_mb"])
def test_window_decomposition(name, dtype, ragged):
    kinds = _decomposes(_run(name, dtype, ragged))
    assert kinds[0] == "gemv" and kinds[-1] in ("post_tail", "tail")


@pytest.mark.parametrize("switches,expect", [
    ({"pair_chain3": 1}, "chain"),
    ({"post_tail": 0}, "tail"),
    ({"wn_chunk": -1}, "wn"),
])
def test_window_decomposition_with_switches(switches, expect):
    make = (lambda sw: _run_shipped(sw)) if "pair_chain3" in switches else (lambda sw: _run("mini", "f16", True, sw))
    kinds = _decomposes(make(switches))
    assert expect in kinds, kinds                # the switch changed the launch sequence the way the GPU's does
    assert expect not in make(None).steps()[1]


def test_window_decomposition_posterior():
    """enc_q followed by flow_forward (mini_q shapes): each entry point decomposes, and the flow runs on enc_q's z."""
    import json
    import os
    import helpers
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_state_dict, make_synthetic_posterior_inputs
    entry = json.load(open(os.path.join(helpers.GOLDEN, "manifest.json")))["mini_q"]
    cfg = entry["config"]
    model = q.SynthesizerTrn(641, 32, **cfg)
    sd = make_synthetic_state_dict(model, entry["weights_seed"])
    spec, g, noise = make_synthetic_posterior_inputs(entry["batch"], entry["frames"], 641, cfg["inter_channels"], cfg["gin_channels"],
                                                     seed0=entry["inputs_seed0"])
    rq, rf = E.window_runs_posterior(model.model_config, sd, spec, g, noise=noise)
    kq = _decomposes(rq)
    assert kq[0] == "gemv" and kq[-1] in ("conv", "sample")
    Nq, _ = rq.steps()
    z = rq.run(0, Nq, E.junk_snapshot(rq))[1]
    ws0 = E.junk_snapshot(rf)[0]
    Nf, kf = rf.steps()
    whole = rf.run(0, Nf, (ws0, z))
    for n in range(Nf + 1):
        part = rf.run(0, n, (ws0, z))
        rest = rf.run(n, Nf, part)
        assert torch.equal(rest[0], whole[0]) and torch.equal(rest[1], whole[1]), n
    assert not torch.equal(whole[1], z)


# ------------------------------------------------------------------ the comparator
@pytest.fixture(scope="module")
def emulated_step():
    """A ResBlock pair launch of the mini config (f16, ragged [T-3, 2] at T = 70): the snapshot after it, and where."""
    run = _run("mini", "f16", True, T=70, B=2)
    N, kinds = run.steps()
    n = len(kinds) - 1 - kinds[::-1].index("pair3")       # the last pair launch: stage 1, 20 frames per unit frame
    before = run.run(0, n, E.junk_snapshot(run))
    after = run.run(n, n + 1, before)
    bufs = E.workspace_map(run.emu, run.cfg, run.B, run.T) + [S.output_spec(run.B, run.out_numel())]
    found = S.compare_snapshots(before, after, bufs, run.B, run.lens.tolist())
    assert found, "the pair launch wrote nothing"
    # the stream it wrote: an f16 buffer at 20 frames per unit frame
    name = max(found, key=lambda e: e["n_diff"])["buffer"]
    buf = next(b for b in bufs if b["name"] == name)
    assert buf["elem"] == "f16" and buf["mul"] == 20
    return run, bufs, buf, after


def _tamper(snap, buf, B, fn):
    ws, out = snap[0].clone(), snap[1].clone()
    v = ws[buf["offset"]:buf["offset"] + buf["bytes"]].view(torch.float16).reshape(buf["groups"], B, buf["rows"], buf["channels"])
    fn(v)
    return ws, out


def _check(run, bufs, ref, got):
    found = S.compare_snapshots(ref, got, bufs, run.B, run.lens.tolist())
    return S.violations(found, "pair3", S.BOUNDS)


def test_comparator_flags_one_frame_of_a_tile(emulated_step):
    run, bufs, buf, after = emulated_step
    def fn(v):
        v[0, 0, 63] = v[0, 0, 62]                      # the last frame of the second 32-frame tile <- its neighbour
    bad = _check(run, bufs, after, _tamper(after, buf, run.B, fn))
    assert len(bad) == 1 and bad[0]["buffer"] == buf["name"]
    w = bad[0]["where"]
    assert (w["b"], w["frame"], w["frame_mod32"]) == (0, 63, 31)
    assert "frame 63 (mod 32: 31" in S.describe(bad[0])


def test_comparator_flags_one_fragment_scaled(emulated_step):
    run, bufs, buf, after = emulated_step
    def fn(v):
        v[0, 0, 64:96, 16:32] *= 1.0 + 2.0 ** -8        # one 16-channel fragment of one 32-frame range, 0.4 % off
    bad = _check(run, bufs, after, _tamper(after, buf, run.B, fn))
    assert len(bad) == 1
    w = bad[0]["where"]
    assert w["b"] == 0 and 64 <= w["frame"] < 96 and 16 <= w["channel"] < 32


def test_comparator_flags_junk_in_valid_rows_only(emulated_step):
    run, bufs, buf, after = emulated_step
    valid = S.valid_rows(buf, run.lens.tolist(), run.B)
    assert valid[1] == 2 * 20 and valid[0] == 67 * 20
    def past_end(v):
        v[0, 1, valid[1]:] = 1234.0                     # past member 1's end: free for a kernel to leave anything there
        v[0, 0, valid[0]:] = float("nan")
    assert _check(run, bufs, after, _tamper(after, buf, run.B, past_end)) == []
    def inside(v):
        v[0, 1, valid[1] - 1, 5] = 1234.0               # the last valid row of the 2-frame member
    bad = _check(run, bufs, after, _tamper(after, buf, run.B, inside))
    assert len(bad) == 1 and (bad[0]["where"]["b"], bad[0]["where"]["frame"], bad[0]["where"]["channel"]) == (1, valid[1] - 1, 5)


def test_comparator_ignores_realistic_noise(emulated_step):
    """Sparse one-ulp flips of stored f16 values, at the rate measured on the MI355X (profiles/r05_step_parity.txt),
    and fp32 differences at the measured relative size, pass."""
    run, bufs, buf, after = emulated_step
    gen = torch.Generator().manual_seed(5)
    ws, out = after[0].clone(), after[1].clone()
    bits = ws[buf["offset"]:buf["offset"] + buf["bytes"]].view(torch.int16)
    n = bits.numel()
    k = max(1, int(n * S.BOUNDS["pair3"]["frac_measured"]))
    idx = torch.randperm(n, generator=gen)[:k]
    sign = torch.where(bits[idx] < 0, -1, 1).to(torch.int16)
    step = torch.where(torch.rand(k, generator=gen) < 0.5, 1, -1).to(torch.int16)
    bits[idx] = bits[idx] + sign * step
    assert _check(run, bufs, after, (ws, out)) == []
    # fp32: the waveform buffer perturbed at a quarter of the pair kind's fp32 bound
    out2 = out.clone()
    rms = float(out2.double().pow(2).mean().sqrt())
    if rms > 0:
        out2 += (torch.rand(out2.shape, generator=gen) - 0.5) * 0.5 * S.BOUNDS["pair3"]["rel"] * rms
        assert _check(run, bufs, after, (ws, out2)) == []
