"""Every row of tests/config_space.py on an MI355X (run with -m gpu): the model geometries validate() accepts, at tiny
shapes, against the fp32 oracle and against the host emulation launch by launch.

Shapes: B 2, T 23 (a multiple of no tile size), and one ragged call with lengths [23, 9] (9 ends inside the first tile
of every stage) whose padding is junk for the units and NaN for the noise.

Tolerances (the project's, tests/test_gpu_parity.py): f16 stages (enc_p -> z_p, flow_reverse -> z, each fed the oracle's
input for that stage) >= 50 dB, f16 waveform >= 45 dB per utterance; the full-length member of the ragged call
torch.equal to the plain batch, the short member >= 100 dB against that utterance converted alone and exactly zero
after its end.  bf16x: waveform >= 40 dB (BASELINE.json's bar), asserted where the bf16x EMULATION of the row
(config_space.ROWS[...]["emu_bf16x"], measured on the host and kept fresh by tests/test_config_space_host.py) reaches
43 dB: GPU and emulation differ by accumulation order only, 3 dB is the margin for that.  Rows whose emulation is below
43 dB run in f16 only and are listed by test_rows_that_run_in_f16_only.

Per launch, for the ragged f16 call: the GPU's buffers after every step against the emulation's replay of that step from
the GPU's own snapshot (tests/test_gpu_step_parity.py's method), with the comparator and the bounds of
tests/stepcheck.py unchanged.  stepcheck.BOUNDS has no entry for the single-band kinds post_tail1 / tail1: they get the
bounds of their four-band siblings post_tail / tail (the same kernels without the band synthesis, an fp32 waveform).
A waveform SNR cannot see one wrong frame at a tile edge; this comparison can.
"""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

import config_space as CS
import emu as E
import stepcheck as S
from helpers import snr_db

pytestmark = pytest.mark.gpu

DEBUG_DEFAULTS = {"post_tail": 1, "post_tail_nf": 4, "pair_wide_launch": 1, "pair_cm4": 1, "conv_cl": 1, "wn_chunk": 0,
                  "pair_chain3": 0, "wn_kernel": 0, "launch_stop": -1}
BF16X_EMU_MIN_DB = 43.0
BOUNDS = dict(S.BOUNDS, post_tail1=S.BOUNDS["post_tail"], tail1=S.BOUNDS["tail"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from quickvc_official_amd import lib as L
    l = L.load_library()                       # raises if the HIP library is missing: no fallback
    assert l.qvc_device_check() == 0
    return l


@pytest.fixture(autouse=True)
def _debug_switches_at_defaults():
    from quickvc_official_amd import lib as L
    for k, v in DEBUG_DEFAULTS.items():
        L.debug_set(k, v)
    yield
    for k, v in DEBUG_DEFAULTS.items():
        L.debug_set(k, v)


def _fm(t):
    return t.transpose(1, 2).contiguous()


def _padded(name):
    """The row's inputs as a ragged batch of lengths CS.RAGGED: junk units and NaN noise past each member's end."""
    unit, g, noise = CS.inputs(name)
    unit, noise = unit.clone(), noise.clone()
    for b, n in enumerate(CS.RAGGED):
        unit[b, :, n:] = 300.0 * (b + 1)
        noise[b, :, n:] = float("nan")
    return unit, g, noise


def _every_launch(name, mc, sd, dev):
    """Ragged f16 call, every launch against the emulation -> (kinds, kernel names)."""
    from test_gpu_step_parity import GpuRun
    unit, g, noise = _padded(name)
    r = E.window_run(mc, sd, unit, g, noise, dtype="f16", lens=CS.RAGGED)
    gpu = GpuRun(r, dev)
    N, kinds = r.steps()
    snaps = [gpu.run(n) for n in range(N + 1)]
    assert gpu.L.debug_get("launch_steps") == N, (gpu.L.debug_get("launch_steps"), N)
    full = gpu.run(-1)
    assert torch.equal(snaps[N][0], full[0]) and torch.equal(snaps[N][1], full[1]), "launch_stop = N differs from a whole run"
    names = gpu.kernel_names()
    assert len(names) == N, (len(names), N)
    bufs = E.workspace_map(r.emu, r.cfg, r.B, r.T) + [S.output_spec(r.B, r.out_numel())]

    def same_bytes(x, y, buf):
        if buf["name"] == "out":
            return torch.equal(x[1].view(torch.int32), y[1].view(torch.int32))
        lo, hi = buf["offset"], buf["offset"] + buf["bytes"]
        return torch.equal(x[0][lo:hi], y[0][lo:hi])

    def one(n):
        ref, got = r.run(n, n + 1, snaps[n]), snaps[n + 1]
        # a launch writes a few buffers: the comparator (which finds nothing in a bit-identical buffer) sees only the others
        return S.compare_snapshots(ref, got, [buf for buf in bufs if not same_bytes(ref, got, buf)], r.B, CS.RAGGED)

    with ThreadPoolExecutor(max_workers=8) as ex:
        results = list(ex.map(one, range(N)))
    failures = []
    for n, found in enumerate(results):
        for e in S.violations(found, kinds[n], BOUNDS, S.SCRATCH.get(kinds[n], ()), "f16"):
            failures.append(f"step {n} ({kinds[n]}: {names[n]}): {S.describe(e)}")
    assert not failures, f"{name}: {len(failures)} buffer(s) out of bounds\n" + "\n".join(failures[:20])
    return kinds, names


@pytest.mark.parametrize("name", list(CS.ROWS))
def test_row_on_the_gpu(lib, dev, name):
    """Every figure is measured and printed first; the assertions come together at the end."""
    from quickvc_official_amd.engine import QvcEngine
    cfg, mc, sd = CS.problem(name)
    row = CS.ROWS[name]
    unit, g, noise = CS.inputs(name)
    ref, taps = CS.reference(name)
    spf = CS.samples_per_frame(cfg)
    eng = QvcEngine(dict(mc, operand_dtype="f16"), sd, dev)
    assert eng.samples_per_frame == spf
    # stage by stage, each fed the oracle's input for that stage
    z_p = eng.enc_p(unit, noise)
    z = eng.flow_reverse(_fm(taps["enc_p.z_p"]), g)
    full = eng.infer_batch(unit.to(dev), g.to(dev), noise.to(dev))
    torch.cuda.synchronize()
    assert full.shape == ref.shape
    db = dict(z_p=snr_db(_fm(taps["enc_p.z_p"]), z_p.cpu()), z=snr_db(_fm(taps["flow.flows.0.out"]), z.cpu()),
              f16=[snr_db(ref[b], full[b].cpu()) for b in range(CS.B)])
    print(f"{name}: GPU f16 z_p {db['z_p']:.1f} dB, z {db['z']:.1f} dB, waveform {[round(v, 1) for v in db['f16']]} dB")
    # the ragged call
    pad_u, _g, pad_n = _padded(name)
    rag = eng.infer_batch_ragged(pad_u.to(dev), g.to(dev), pad_n.to(dev), torch.tensor(CS.RAGGED, dtype=torch.int32))
    n = CS.RAGGED[1]
    alone = eng.infer_batch(unit[1:2, :, :n].to(dev), g[1:2].to(dev), noise[1:2, :, :n].to(dev))
    torch.cuda.synchronize()
    db["ragged_alone"] = snr_db(alone[0].cpu(), rag[1, :, :n * spf].cpu())
    db["ragged_past_end"] = float(rag[1, :, n * spf:].abs().max())
    db["ragged_full_equal"] = bool(torch.equal(rag[0], full[0]))
    print(f"{name}: ragged: member 0 equal {db['ragged_full_equal']}, member 1 vs alone {db['ragged_alone']:.1f} dB, max past its end {db['ragged_past_end']}")
    # the mixed operand mode, where its emulation says the bar is within reach
    emu_x = row["emu_bf16x"]
    assert emu_x is not None or not row["emulated"], "tests/test_config_space_host.py measures emu_bf16x"
    if emu_x is not None and min(emu_x) >= BF16X_EMU_MIN_DB:
        engx = QvcEngine(dict(mc, operand_dtype="bf16x"), sd, dev)
        outx = engx.infer_batch(unit.to(dev), g.to(dev), noise.to(dev))
        torch.cuda.synchronize()
        db["bf16x"] = [snr_db(ref[b], outx[b].cpu()) for b in range(CS.B)]
        print(f"{name}: GPU bf16x waveform {[round(v, 1) for v in db['bf16x']]} dB (emulation {emu_x})")
    else:
        print(f"{name}: f16 only -- bf16x emulation: {emu_x if emu_x is not None else 'none (the emulation refuses the single-band decoder)'}")
    # every launch of the ragged call against the emulation
    step_failure, names = None, None
    if row["emulated"]:
        try:
            _kinds, names = _every_launch(name, mc, sd, dev)
            print(f"{name}: {len(names)} launches: {' '.join(names)}")
        except AssertionError as e:
            step_failure = str(e)
            print(step_failure)
    else:
        # stepcheck replays launches on the emulation, whose backend is frozen before the single-band decoder and refuses
        # it (tests/test_istft_single_band.py): this row keeps the oracle's assertions only
        print(f"{name}: no per-launch comparison (single-band decoder)")
    path = os.environ.get("QVC_CONFIG_SPACE_LOG")
    if path:
        with open(path, "a") as f:
            f.write(repr(dict(name=name, db=db, names=names, step_failure=step_failure)) + "\n")
    assert db["z_p"] >= 50.0 and db["z"] >= 50.0, db
    assert min(db["f16"]) >= 45.0, db
    assert bool(torch.isfinite(rag).all())
    assert db["ragged_full_equal"], "the full-length member of the ragged batch differs from the plain batch"
    assert db["ragged_alone"] >= 100.0 and db["ragged_past_end"] == 0.0, db
    assert "bf16x" not in db or min(db["bf16x"]) >= 40.0, db
    assert step_failure is None, step_failure


STACK_BATCH = 65     # more than 64 tiles of 32 frames: launch_wn_stack_typed leaves the 16-frame tile of tiny batches


@pytest.mark.parametrize("name", ["wn_k3", "wn_enc3_flow2", "wn_enc1_flow1", "wn_flows2"])
def test_wn_stacks_in_the_32_frame_window(lib, dev, name):
    """At B 2 x T 23 a whole-stack launch whose halo fits takes the 16-frame tile the library keeps for tiny batches, so
    the rows above run the 3-fragment window (32 output frames) only where the halo is too wide for it.  Here the WaveNet
    half alone (enc_p -> z_p, flow_reverse -> z; no decoder) runs at 65 utterances of 23 frames -- 65 tiles, one more than
    the tiny-batch rule allows -- for taps 3, stacks of 1, 2 and 3 layers and the reference's geometry in the generic
    kernel.  Bars: the stage bars, >= 50 dB against the oracle in f16."""
    import qvc_oracle as oracle
    from quickvc_official_amd.engine import QvcEngine
    from quickvc_official_amd.synth import make_synthetic_inputs
    cfg, mc, sd = CS.problem(name)
    H, C = cfg["hidden_channels"], cfg["inter_channels"]
    unit, g, noise = make_synthetic_inputs(STACK_BATCH, CS.T, 256, C, cfg["gin_channels"], seed0=CS.INPUTS_SEED)
    wn = oracle.wn_geometry(cfg)
    sdf = {k: v.float() for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()}
    with torch.no_grad():
        z_p, _mu, _logs = oracle.cond_normal_wn(sdf, "enc_p", unit, noise, H, C, None, None, wn["kernel_size"], wn["enc_layers"])
        z = oracle.flow_reverse(sdf, z_p, g.unsqueeze(-1), C, H, wn["n_flows"], None, wn["kernel_size"], wn["flow_layers"])
    eng = QvcEngine(dict(mc, operand_dtype="f16"), sd, dev)
    got_p = eng.enc_p(unit, noise)
    got_z = eng.flow_reverse(_fm(z_p), g)
    torch.cuda.synchronize()
    db = (snr_db(_fm(z_p), got_p.cpu()), snr_db(_fm(z), got_z.cpu()))
    print(f"{name}: B {STACK_BATCH}: z_p {db[0]:.1f} dB, z {db[1]:.1f} dB")
    assert min(db) >= 50.0, db
    worst = min(snr_db(_fm(z)[b], got_z[b].cpu()) for b in range(STACK_BATCH))
    assert worst >= 45.0, worst                                  # no single utterance (tile) far off the average


def test_rows_that_run_in_f16_only():
    """The rows the bf16x assertion leaves out, with the emulated value that decides it -- listed, not skipped silently."""
    left_out = {name: row["emu_bf16x"] for name, row in CS.ROWS.items() if row["emu_bf16x"] is None or min(row["emu_bf16x"]) < BF16X_EMU_MIN_DB}
    for name, v in left_out.items():
        print(f"{name}: f16 only, bf16x emulation {v if v is not None else 'none (single-band decoder: not emulated)'}")
    assert all(v is not None or not CS.ROWS[name]["emulated"] for name, v in left_out.items())
    assert len(left_out) <= len(CS.ROWS) // 2, left_out          # bf16x is the mode the benchmark runs: most rows must cover it
