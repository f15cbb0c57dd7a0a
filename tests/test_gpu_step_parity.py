"""Every launch of the hot path against its host-emulated twin, step by step (run with -m gpu on an MI355X).

The product path is stopped after each of its steps (debug switch launch_stop = n: only steps [0, n) are issued, into
a caller-owned workspace and output that start from the same junk bytes every time), and both buffers are copied to
the host.  Step n is then replayed on the host emulation (oracle/qvc_emu.cpp: the same Path<> over the same packed
blob, fp64 accumulation, operands and stored streams rounded where the kernels round them) from GPU snapshot n, and
its result is compared with GPU snapshot n + 1: every workspace buffer over its valid rows, and the output.  Identical
input bytes leave only fp32 accumulation order, transcendental implementations and rare one-ulp flips of a stored
2-byte value between the two, so the bar holds at every element instead of on average.

Tolerances (measured first: profiles/r05_step_parity.txt), per step kind, from stepcheck.BOUNDS:
2-byte outputs at most `ulp` ulps apart with at most a fraction `over1` of the valid elements more than one ulp off;
fp32 outputs within `rel` of the buffer's RMS.  Buffers a kernel uses as private scratch are listed in
stepcheck.SCRATCH.

Sanity checks the method rests on: the GPU and the emulation count the same steps; launch_stop = N is bit-identical to
an unrestricted run; two runs to N are bit-identical (the GPU path is deterministic).
"""
import ctypes
import json
import os
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

import emu as E
import stepcheck as S
from helpers import load_case, regenerate

pytestmark = pytest.mark.gpu

SWITCH_DEFAULTS = {"post_tail": 1, "post_tail_nf": 4, "pair_wide_launch": 1, "pair_cm4": 1, "conv_cl": 1, "wn_chunk": 0,
                   "pair_chain3": 0, "wn_kernel": 0, "launch_stop": -1}
JUNK = 0x3C          # starting bytes of workspace and output: f16 1.06, fp32 0.0115 (finite, never a plausible result)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _switches_restored():
    from quickvc_official_amd import lib as L
    for k, v in SWITCH_DEFAULTS.items():
        L.debug_set(k, v)
    yield
    for k, v in SWITCH_DEFAULTS.items():
        L.debug_set(k, v)


class GpuRun:
    """One whole-path entry point on the device, into a caller-owned workspace and output."""

    def __init__(self, emu_run, dev, init_out=None):
        from quickvc_official_amd import lib as L
        self.L, self.hip, self.r, self.dev = L, L.load_library(), emu_run, dev
        self.blob = emu_run.blob.to(dev)
        self.inputs = [x.to(dev) for x in emu_run.inputs]
        self.lens = None if emu_run.lens is None else emu_run.lens.to(dev)
        self.ws = torch.empty(emu_run.n_ws, dtype=torch.uint8, device=dev)
        self.out = torch.empty(emu_run.out_numel(), dtype=torch.float32, device=dev)
        self.init_out = init_out

    def run(self, stop):
        """Snapshot (workspace, output) on the host after the steps [0, stop) (stop = -1: all)."""
        r, hip = self.r, self.hip
        self.ws.fill_(JUNK)
        if self.init_out is None:
            self.out.view(torch.uint8).fill_(JUNK)
        else:
            self.out.copy_(self.init_out)
        self.L.debug_set("launch_stop", stop)
        cfgp = ctypes.byref(r.cfg)
        torch.cuda.synchronize()
        if r.kind == "infer":
            unit, g, noise = self.inputs
            if self.lens is None:
                st = hip.qvc_infer_batch(cfgp, self.blob.data_ptr(), unit.data_ptr(), g.data_ptr(), noise.data_ptr(), self.out.data_ptr(),
                                         r.B, r.T, self.ws.data_ptr(), r.n_ws, None)
            else:
                st = hip.qvc_infer_batch_ragged(cfgp, self.blob.data_ptr(), unit.data_ptr(), g.data_ptr(), noise.data_ptr(),
                                                self.out.data_ptr(), r.B, r.T, self.lens.data_ptr(), self.ws.data_ptr(), r.n_ws, None)
        elif r.kind == "enc_q":
            spec, g, noise = self.inputs
            st = hip.qvc_enc_q(cfgp, self.blob.data_ptr(), spec.data_ptr(), g.data_ptr(), noise.data_ptr(), self.out.data_ptr(),
                               r.B, r.T, self.ws.data_ptr(), r.n_ws, None)
        else:
            (g,) = self.inputs
            st = hip.qvc_flow_forward(cfgp, self.blob.data_ptr(), self.out.data_ptr(), g.data_ptr(), r.B, r.T, self.ws.data_ptr(), r.n_ws, None)
        torch.cuda.synchronize()
        self.L.debug_set("launch_stop", -1)
        assert st == 0, hip.qvc_status_string(st)
        return self.ws.cpu(), self.out.cpu()

    def kernel_names(self):
        """Launch names of the timed twin (plain batch, same shapes) -- one per step of the conversion path."""
        r, hip = self.r, self.hip
        if r.kind != "infer":
            return None
        unit, g, noise = self.inputs
        recs = (self.L.QvcLaunchRecord * 4096)()
        n = ctypes.c_int32(0)
        self.ws.fill_(JUNK)
        st = hip.qvc_infer_batch_timed(ctypes.byref(r.cfg), self.blob.data_ptr(), unit.data_ptr(), g.data_ptr(), noise.data_ptr(),
                                       self.out.data_ptr(), r.B, r.T, self.ws.data_ptr(), r.n_ws, None, recs, 4096, ctypes.byref(n))
        torch.cuda.synchronize()
        assert st == 0, hip.qvc_status_string(st)
        return [recs[i].name.decode() for i in range(n.value)]


def _log(case, rows):
    path = os.environ.get("QVC_STEP_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            for row in rows:
                f.write(json.dumps(dict(case=case, **row)) + "\n")


def _check_steps(case, emu_run, gpu):
    N, kinds = emu_run.steps()
    full = gpu.run(-1)
    assert gpu.L.debug_get("launch_steps") == N, (gpu.L.debug_get("launch_steps"), N)
    names = gpu.kernel_names() or kinds
    assert len(names) == N, (len(names), N)
    snaps = [gpu.run(n) for n in range(N + 1)]
    assert torch.equal(snaps[N][0], full[0]) and torch.equal(snaps[N][1], full[1]), "launch_stop = N differs from a whole run"
    again = gpu.run(N)
    assert torch.equal(again[0], full[0]) and torch.equal(again[1], full[1]), "the GPU path is not deterministic"
    del again, full
    bufs = E.workspace_map(emu_run.emu, emu_run.cfg, emu_run.B, emu_run.T) + [S.output_spec(emu_run.B, emu_run.out_numel())]
    lens = None if emu_run.lens is None else emu_run.lens.tolist()

    def one(n):
        ref = emu_run.run(n, n + 1, snaps[n])
        return S.compare_snapshots(ref, snaps[n + 1], bufs, emu_run.B, lens)

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        results = list(ex.map(one, range(N)))
    rows, failures = [], []
    for n, found in enumerate(results):
        kind = kinds[n]
        for e in found:
            rows.append(dict(step=n, kind=kind, kernel=names[n], dtype=emu_run.dtype, **{k: e[k] for k in ("buffer", "elem", "max", "frac", "n_over1", "n_valid")}))
        for e in S.violations(found, kind, S.BOUNDS, S.SCRATCH.get(kind, ()), emu_run.dtype):
            failures.append(f"step {n} ({kind}: {names[n]}): {S.describe(e)}")
    _log(case, rows)
    assert not failures, f"{case}: {len(failures)} buffer(s) out of bounds\n" + "\n".join(failures[:20])
    return kinds


def _shipped(seed=901):
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_state_dict, make_synthetic_inputs
    cfg = dict(q.DEFAULT_MODEL_CONFIG)
    model = q.SynthesizerTrn(641, 32, **cfg)
    sd = make_synthetic_state_dict(model, seed)
    lens = [70, 33, 2]
    unit, g, noise = make_synthetic_inputs(3, 70, 256, cfg["inter_channels"], cfg["gin_channels"], seed0=seed)
    for b, n in enumerate(lens):
        unit[b, :, n:] = 300.0 * (b + 1)           # junk the path must never read unmasked
        noise[b, :, n:] = -55.0
    return model.model_config, sd, unit, g, noise, lens


SHIPPED_CASES = [("f16", {}), ("bf16x", {}), ("bf16", {}),
                 ("f16", {"wn_kernel": 1}), ("f16", {"wn_kernel": 2}), ("f16", {"wn_kernel": 3}), ("f16", {"pair_chain3": 1}),
                 ("f16", {"post_tail": 0}), ("f16", {"post_tail_nf": 2}), ("f16", {"wn_chunk": -1})]


@pytest.mark.parametrize("dtype,switches", SHIPPED_CASES, ids=[d + "".join(f"-{k}={v}" for k, v in s.items()) for d, s in SHIPPED_CASES])
def test_shipped_config_ragged_every_launch(dev, dtype, switches):
    """Shipped config, ragged batch [70, 33, 2]: a partial 32- and 64-frame tile, ends inside halos, a 2-frame member."""
    from quickvc_official_amd import lib as L
    mc, sd, unit, g, noise, lens = _shipped()
    for k, v in switches.items():
        L.debug_set(k, v)
    emu_switches = {k: v for k, v in switches.items() if k in E.SWITCH_DEFAULTS}
    r = E.window_run(mc, sd, unit, g, noise, dtype=dtype, lens=lens, switches=emu_switches)
    kinds = _check_steps(f"shipped-{dtype}-{switches}", r, GpuRun(r, dev))
    if "pair_chain3" in switches:
        assert "chain" in kinds
    if "wn_chunk" in switches:
        assert "wn" in kinds and "wn_stack" not in kinds
    if "post_tail" in switches:
        assert "tail" in kinds and "post_tail" not in kinds


def _other(name):
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_state_dict, make_synthetic_inputs
    over = {
        "wide": dict(inter_channels=64, hidden_channels=256, upsample_initial_channel=832, gin_channels=32),
        "narrow": dict(inter_channels=128, hidden_channels=96, upsample_initial_channel=256, gin_channels=128),
        "x4x4": dict(upsample_rates=[4, 4], upsample_kernel_sizes=[15, 16], resblock_kernel_sizes=[3, 5, 7],
                     resblock_dilation_sizes=[[1, 2, 3], [1, 2, 3], [1, 2, 3]], upsample_initial_channel=384),
        "multiband": dict(ms_istft_vits=False, mb_istft_vits=True, upsample_initial_channel=256, inter_channels=96, hidden_channels=128),
        "mini256": dict(inter_channels=256, hidden_channels=64, upsample_initial_channel=128, gin_channels=64),
    }[name]
    cfg = dict(q.DEFAULT_MODEL_CONFIG, **over)
    model = q.SynthesizerTrn(641, 32, **cfg)
    sd = make_synthetic_state_dict(model, 311)
    unit, g, noise = make_synthetic_inputs(2, 24, 256, cfg["inter_channels"], cfg["gin_channels"], seed0=71)
    return model.model_config, sd, unit, g, noise


@pytest.mark.parametrize("name", ["wide", "narrow", "x4x4", "multiband", "odd", "mini256"])
def test_other_configs_every_launch(dev, name):
    """Other configurations, plain batch, f16: the unfused conv1 / conv2 fallback with its 2-byte residual and WaveNet
    width 256 (wide), up-samplers that are not lane-packed and other proj pairings (narrow, x4x4), the PQMF tail
    (multiband), odd channel counts (the odd golden config), natural proj rows with the separate sample launch (the
    mini config at inter 256)."""
    if name == "odd":
        entry, _ = load_case("odd")
        model, sd, unit, g, noise = regenerate(entry)
        mc = model.model_config
    else:
        mc, sd, unit, g, noise = _other(name)
    r = E.window_run(mc, sd, unit, g, noise, dtype="f16")
    kinds = _check_steps(f"{name}-f16", r, GpuRun(r, dev))
    if name == "wide":
        assert kinds.count("conv") > 5
    if name == "mini256":
        assert "sample" in kinds


def test_posterior_every_launch(dev):
    """enc_q then flow_forward on the mini_q shapes, f16."""
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
    gq = GpuRun(rq, dev)
    _check_steps("mini_q-enc_q-f16", rq, gq)
    z = gq.run(-1)[1].to(dev)
    _check_steps("mini_q-flow_forward-f16", rf, GpuRun(rf, dev, init_out=z))
