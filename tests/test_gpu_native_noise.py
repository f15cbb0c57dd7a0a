"""GPU tests (run with -m gpu on an MI355X) of the noise drawn on the device: the counter-based generator of
include/qvc.h (qvc_noise_rng) at its three draw sites -- the EPI_SAMPLE epilogue of the projection, sample_rng_kernel
(natural projection rows) and sample_rows_rng_kernel (fan-out) -- behind qvc_infer_batch_ragged_rng[_fm],
qvc_infer_fanout_ragged_rng[_fm] and qvc_stream_step_rng, with qvc_noise_fill as the bridge to the pointer forms.

Bars:
  * qvc_noise_fill against the float64 numpy restatement (tests/test_native_noise_host.py): max abs error <= 1.5e-5.
    |r| <= sqrt(48 ln 2) = 5.77; the fp32 rounding of 2 pi u2 is <= 3.7e-7 rad; logf, sqrtf, sinf, cosf are each within
    2 ulp: together about 6e-6, so the bar carries 2.5x headroom.  Measured on an MI355X: see DESIGN.md section 5h;
  * fused against materialised, batch independence, fan-out against the expanded batch, the scales: torch.equal -- the
    draw is one inlined function with contraction off, a normal crosses memory in fp32 unrounded, and gauss_sample is
    the shared helper of every draw site;
  * streaming against the offline call: >= 90 dB per stream, the bar of the other streaming tests;
  * against the fp32 oracle fed the qvc_noise_fill tensor: f16 >= 50 dB, bf16x >= 40 dB.
Shapes: B 2 x T 23 and ragged [23, 9] (tests/config_space.py) on the mini model and two rows of the configuration table.
"""
import ctypes
import json

import numpy as np
import pytest
import torch

import config_space as CS
import emu as E
import qvc_oracle as oracle
import test_native_noise_host as NH
from helpers import snr_db
from test_gpu_memory_contract import NAN, PathCase, _ptr, _stream, drive

pytestmark = pytest.mark.gpu

SEED = 0x5EEDC0DE12345678
DEBUG_DEFAULTS = {"post_tail": 1, "post_tail_nf": 4, "pair_wide_launch": 1, "pair_cm4": 1, "conv_cl": 1, "wn_chunk": 0,
                  "pair_chain3": 0, "wn_kernel": 0, "launch_stop": -1}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from quickvc_official_amd import lib as L
    l = L.load_library()
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


_PROBLEMS = {}


def _problem(name):
    """(constructor config, model_config, state dict) of 'mini' (MINI_MODEL_CONFIG: paired projection rows) or a row of
    tests/config_space.py; built once."""
    if name not in _PROBLEMS:
        if name == "mini":
            import quickvc_official_amd as q
            from quickvc_official_amd.synth import make_synthetic_state_dict
            cfg = dict(q.MINI_MODEL_CONFIG)
            model = q.SynthesizerTrn(641, 32, **cfg)
            _PROBLEMS[name] = (cfg, model.model_config, make_synthetic_state_dict(model, CS.WEIGHTS_SEED))
        else:
            _PROBLEMS[name] = CS.problem(name)
    return _PROBLEMS[name]


def _inputs(name, batch=CS.B, frames=CS.T, seed0=CS.INPUTS_SEED):
    from quickvc_official_amd.synth import make_synthetic_inputs
    cfg = _problem(name)[0]
    unit, g, _noise = make_synthetic_inputs(batch, frames, 256, cfg["inter_channels"], cfg["gin_channels"], seed0=seed0)
    return unit, g


_ENGINES = {}


def _engine(name, dev, dtype="f16"):
    from quickvc_official_amd.engine import QvcEngine
    if (name, dtype) not in _ENGINES:
        _cfg, mc, sd = _problem(name)
        _ENGINES[(name, dtype)] = QvcEngine(dict(mc, operand_dtype=dtype), sd, dev)
    return _ENGINES[(name, dtype)]


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


# ------------------------------------------------------------------ 1. the draw itself
def test_noise_fill_matches_the_restatement(lib, dev):
    eng = _engine("mini", dev)
    keys = [7, 2 ** 64 - 3, 0x100000002]
    got = eng.noise_fill(SEED, keys, 32, 64, frame0=5)
    torch.cuda.synchronize()
    want = NH.noise_tensor(SEED, keys, 32, 64, frame0=5)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print(f"qvc_noise_fill vs the float64 restatement: max abs error {err:.3e}")
    assert got.shape == (3, 32, 64) and err <= 1.5e-5, err
    # frame0 and the scale are what the restatement says they are, bit for bit on the device's own values
    assert torch.equal(eng.noise_fill(SEED, keys, 32, 20, frame0=25), got[:, :, 20:40])
    assert torch.equal(eng.noise_fill(SEED, keys, 32, 64, frame0=5, scale=0.5), 0.5 * got)
    assert torch.equal(eng.noise_fill(SEED, keys[:1], 8, 64, frame0=5), got[:1, :8])
    # a frame count that is no multiple of the 256-thread block, frames near 2^31
    big = eng.noise_fill(SEED, [7], 8, 300, frame0=2 ** 31 - 150)
    want_big = NH.noise_tensor(SEED, [7], 8, 300, frame0=2 ** 31 - 150)
    torch.cuda.synchronize()
    assert float(np.abs(big.cpu().numpy().astype(np.float64) - want_big).max()) <= 1.5e-5


# ------------------------------------------------------------------ 2. fused == materialised
@pytest.mark.parametrize("name", ["mini", "inter256_h8", "ch104"])
def test_fused_draw_equals_the_materialised_tensor(lib, dev, name):
    """mini: the projection's sampling epilogue; inter256_h8: natural rows + sample_rng_kernel; ch104: inter 72, whose last
    fragment holds two 4-channel groups and not four."""
    cfg, _mc, _sd = _problem(name)
    eng = _engine(name, dev)
    info = (ctypes.c_int32 * 8)()
    assert lib.qvc_plan_info(ctypes.byref(eng.cfg), info) == 0
    assert info[0] == (0 if name == "inter256_h8" else 1), list(info)
    C = cfg["inter_channels"]
    unit, g = _inputs(name)
    unit, g = unit.to(dev), g.to(dev)
    keys = [3, 2 ** 40 + 9]
    for lens in ([CS.T, CS.T], CS.RAGGED):
        noise = eng.noise_fill(SEED, keys, C, CS.T)
        fused = eng.infer_batch_ragged(unit, g, None, _i32(lens), rng=(SEED, keys, 1.0)).clone()
        mat = eng.infer_batch_ragged(unit, g, noise, _i32(lens))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(fused).all()) and float(fused.abs().max()) > 0
        assert torch.equal(fused, mat), (name, lens, snr_db(mat.cpu(), fused.cpu()))
    if name == "mini":                                                  # the frame-major twin, once
        fm = eng.infer_batch_ragged(unit.transpose(1, 2).contiguous(), g, None, _i32(CS.RAGGED), unit_fm=True, rng=(SEED, keys, 1.0))
        torch.cuda.synchronize()
        assert torch.equal(fm, fused)


# ------------------------------------------------------------------ 3. independence of the batch
def test_an_utterance_draws_the_same_noise_in_any_batch(lib, dev):
    eng = _engine("mini", dev)
    spf = eng.samples_per_frame
    unit, g = _inputs("mini", batch=3, frames=40, seed0=73)
    unit, g = unit.to(dev), g.to(dev)
    n = 9
    u, gg = unit[1:2, :, :n].contiguous(), g[1:2]                      # the utterance with key 7: 9 frames

    def run(units, gs, lens, keys, seed=SEED):
        out = eng.infer_batch_ragged(units.contiguous(), gs.contiguous(), None, _i32(lens), rng=(seed, keys, 1.0)).clone()
        torch.cuda.synchronize()
        return out
    alone = run(u, gg, [n], [7])
    pair_units = torch.zeros(2, 256, 23, device=dev)
    pair_units[0], pair_units[1, :, :n] = unit[0, :, :23], u[0]
    in_pair = run(pair_units, torch.stack([g[0], gg[0]]), [23, n], [1, 7])
    tri_units = torch.full((3, 256, 40), NAN, device=dev)               # padded to 40, junk in the padding
    tri_units[0, :, :n], tri_units[1, :, :31], tri_units[2] = u[0], unit[0, :, :31], unit[2]
    in_three = run(tri_units, torch.stack([gg[0], g[0], g[2]]), [n, 31, 40], [7, 5, 6])
    want = alone[0, :, :spf * n]
    assert float(want.abs().max()) > 0
    assert torch.equal(in_pair[1, :, :spf * n], want) and torch.equal(in_three[0, :, :spf * n], want)
    assert float(in_pair[1, :, spf * n:].abs().max()) == 0.0 and float(in_three[0, :, spf * n:].abs().max()) == 0.0
    # equal keys in two rows: equal noise, so equal rows for equal inputs
    twice = run(torch.cat([u, u]), torch.cat([gg, gg]), [n, n], [7, 7])
    assert torch.equal(twice[0], twice[1]) and torch.equal(twice[0], alone[0])
    # another key, another seed (either half of it): another draw
    assert not torch.equal(run(u, gg, [n], [8]), alone)
    assert not torch.equal(run(u, gg, [n], [7 + 2 ** 32]), alone)
    assert not torch.equal(run(u, gg, [n], [7], seed=SEED + 1), alone)
    assert not torch.equal(run(u, gg, [n], [7], seed=SEED ^ (1 << 40)), alone)


# ------------------------------------------------------------------ 4. fan-out
@pytest.mark.parametrize("name", ["mini", "inter256_h8"])
def test_fanout_rng_equals_the_expanded_batch(lib, dev, name):
    """U 2, R 5: per-row keys, a map value that needs clamping (on the device), NaN in the unit padding.  Both projection
    routes: EPI_STATS + sample_rows_rng_kernel (mini) and the plain conv + sample_rows_rng_kernel (inter256_h8)."""
    eng = _engine(name, dev)
    spf = eng.samples_per_frame
    unit, g = _inputs(name, batch=5, frames=CS.T, seed0=75)
    lens, raw, clamped = [CS.T, 9], [1, 0, 9, 0, 1], [1, 0, 1, 0, 1]
    src_unit = unit[:2].clone().to(dev)
    src_unit[1, :, 9:] = NAN
    g = g.to(dev)
    keys = [11, 12, 13, 12, 2 ** 63 + 1]                                # rows 1 and 3: same source, same key, other g
    fan = eng.infer_fanout_ragged(src_unit, _i32(lens).to(dev), _i32(raw).to(dev), g, None, rng=(SEED, keys, 1.0)).clone()
    fan_fm = eng.infer_fanout_ragged(src_unit.transpose(1, 2).contiguous(), _i32(lens), _i32(clamped), g, None, unit_fm=True,
                                     rng=(SEED, keys, 1.0)).clone()
    expanded = eng.infer_batch_ragged(src_unit[clamped].contiguous(), g, None, _i32([lens[s] for s in clamped]), rng=(SEED, keys, 1.0))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(fan).all()) and torch.equal(fan, expanded) and torch.equal(fan_fm, expanded)
    for r, s in enumerate(clamped):
        assert float(fan[r, :, :spf * lens[s]].abs().max()) > 0
        if lens[s] < CS.T:
            assert float(fan[r, :, spf * lens[s]:].abs().max()) == 0.0
    assert not torch.equal(fan[1], fan[3])                              # same source and key, another speaker
    with pytest.raises(ValueError):
        eng.infer_fanout_ragged(src_unit, _i32(lens), _i32(clamped), g, None)
    with pytest.raises(ValueError):
        eng.infer_fanout_ragged(src_unit, _i32(lens), _i32(clamped), g, None, rng=(SEED, keys[:4], 1.0))


# ------------------------------------------------------------------ 5. streaming
def _mini_model(dev, dtype="f16"):
    import quickvc_official_amd as q
    cfg, _mc, sd = _problem("mini")
    model = q.SynthesizerTrn(641, 32, **dict(cfg, operand_dtype=dtype))
    model.load_state_dict(sd)
    return model.to(dev).eval()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_streamed_rng_equals_offline_rng(lib, dev, graph):
    """2 streams of 70 and 41 frames at hop 16 through qvc_stream_step_rng, keys set at admission (StreamConverter.start);
    graph: the step captured once and replayed.  Nothing is aligned by the caller: there is no noise tensor."""
    from quickvc_official_amd.streaming import StreamConverter
    model = _mini_model(dev)
    eng = model.engine()
    lens, keys, hop = [70, 41], [2 ** 33 + 4, 9], 16
    unit, g = _inputs("mini", batch=2, frames=70, seed0=77)
    unit, g = unit.to(dev), g.to(dev)
    offline = eng.infer_batch_ragged(unit, g, None, _i32(lens), rng=(SEED, keys, 1.0)).clone()
    assert bool(torch.isfinite(offline).all()) and float(offline[1, :, :41 * eng.samples_per_frame].abs().max()) > 0
    conv = StreamConverter(model, streams=2, hop_frames=hop, use_graph=graph, seed=SEED)
    assert (conv._rng_graph is not None) == graph
    conv.reset(lengths=torch.zeros(2, dtype=torch.int32))              # both slots idle
    for s in range(2):
        conv.start(s, g[s], length=lens[s], key=keys[s])
    spf, lag = conv.spf, conv.lag
    got = torch.zeros(2, 70 * spf, device=dev)
    pad = torch.nn.functional.pad(unit, (0, hop + lag))
    for n in range(-(-(70 + lag) // hop)):
        chunk = conv.step(pad[:, :, n * hop:(n + 1) * hop])
        f0 = n * hop - lag
        lo, hi = max(f0, 0), min(f0 + hop, 70)
        if hi > lo:
            got[:, lo * spf:hi * spf] = chunk[:, (lo - f0) * spf:(hi - f0) * spf]
    torch.cuda.synchronize()
    assert conv.finished(0) and conv.finished(1)
    for s, n in enumerate(lens):
        db = snr_db(offline[s, 0, :n * spf].cpu(), got[s, :n * spf].cpu())
        print(f"stream {s} ({n} frames, graph {graph}): {db:.1f} dB against the offline rng call")
        assert db >= 90.0, (s, db)
        assert float(got[s, n * spf:].abs().max()) == 0.0 if n < 70 else True
    # the convenience form: the same through convert(seed=, keys=)
    whole = conv.convert(unit, g, lengths=_i32(lens), seed=SEED, keys=keys)
    torch.cuda.synchronize()
    for s, n in enumerate(lens):
        assert snr_db(offline[s, 0, :n * spf].cpu(), whole[s, 0, :n * spf].cpu()) >= 90.0, s
    with pytest.raises(ValueError):
        StreamConverter(model, streams=2, hop_frames=hop, use_graph=False).step(pad[:, :, :hop])     # no seed, no noise


def test_stream_slot_readmitted_under_a_new_key(lib, dev):
    """Slot 0 streams 150 frames under key 21 throughout; slot 1 streams 20 frames under key 22, is retired once flushed and
    re-admitted with another utterance (25 frames) under key 23 -- in the captured graph, which only holds the key
    array's pointer.  Each of the three equals its offline rng conversion."""
    from quickvc_official_amd.streaming import StreamConverter
    model = _mini_model(dev)
    eng = model.engine()
    hop = 16
    unit, g = _inputs("mini", batch=3, frames=150, seed0=79)
    unit, g = unit.to(dev), g.to(dev)
    lens, keys = [150, 20, 25], [21, 22, 23]
    offline = eng.infer_batch_ragged(unit, g, None, _i32(lens), rng=(SEED, keys, 1.0)).clone()
    conv = StreamConverter(model, streams=2, hop_frames=hop, use_graph=True, seed=SEED)
    spf, lag = conv.spf, conv.lag
    conv.reset(lengths=torch.zeros(2, dtype=torch.int32))
    occupant = [0, 1]
    for s, i in enumerate(occupant):
        conv.start(s, g[i], length=lens[i], key=keys[i])
    got = {i: torch.zeros(lens[i] * spf, device=dev) for i in range(3)}
    done, steps, readmitted_at = set(), 0, None
    while len(done) < 3:
        u = torch.zeros(2, 256, hop, device=dev)
        for s, i in enumerate(occupant):
            if i is not None:
                p = conv.position(s)
                a, b = p, min(p + hop, lens[i])
                if b > a:
                    u[s, :, :b - a] = unit[i, :, a:b]
        before = [conv.position(s) for s in range(2)]
        out = conv.step(u)
        steps += 1
        for s, i in enumerate(occupant):
            if i is None:
                continue
            f0 = before[s] - lag
            lo, hi = max(f0, 0), min(f0 + hop, lens[i])
            if hi > lo:
                got[i][lo * spf:hi * spf] = out[s, (lo - f0) * spf:(hi - f0) * spf]
            if conv.finished(s):
                done.add(i)
                occupant[s] = None
                if i == 1:                                              # retire, re-admit under a new key
                    conv.start(s, g[2], length=lens[2], key=keys[2])
                    occupant[s], readmitted_at = 2, steps
        assert steps < 40
    torch.cuda.synchronize()
    assert readmitted_at is not None and readmitted_at * hop < lens[0]  # while stream 0 was still being fed
    for i in range(3):
        db = snr_db(offline[i, 0, :lens[i] * spf].cpu(), got[i].cpu())
        assert db >= 90.0, (i, db)


# ------------------------------------------------------------------ 6. the scale
def test_noise_scale(lib, dev):
    eng = _engine("mini", dev)
    unit, g = _inputs("mini")
    unit, g = unit.to(dev), g.to(dev)
    keys, lens, C = [3, 4], _i32(CS.RAGGED), 64
    one = eng.noise_fill(SEED, keys, C, CS.T)

    def rng(scale):
        out = eng.infer_batch_ragged(unit, g, None, lens, rng=(SEED, keys, scale)).clone()
        torch.cuda.synchronize()
        return out

    def ptr(noise):
        out = eng.infer_batch_ragged(unit, g, noise, lens).clone()
        torch.cuda.synchronize()
        return out
    assert torch.equal(rng(0.0), ptr(torch.zeros_like(one)))            # the deterministic mean conversion
    assert torch.equal(rng(1.0), ptr(one))
    assert torch.equal(rng(0.5), ptr(0.5 * one))
    assert not torch.equal(rng(0.5), rng(1.0)) and not torch.equal(rng(0.0), rng(0.5))
    # the model surface: seed / keys / noise_scale; the default keys are 0 .. B-1, the default scale is 1
    model = _mini_model(dev)
    via_model = model.infer_batch(unit, g, seed=SEED, keys=keys, noise_scale=0.5)
    ragged = model.infer_ragged([unit[0], unit[1, :, :9]], g, seed=SEED, keys=keys, noise_scale=0.5)
    torch.cuda.synchronize()
    half = rng(0.5)
    assert torch.equal(via_model[0], eng.infer_batch_ragged(unit, g, None, _i32([CS.T, CS.T]), rng=(SEED, keys, 0.5))[0])
    assert torch.equal(ragged[0], half[0]) and torch.equal(ragged[1], half[1, :, :9 * eng.samples_per_frame])
    with pytest.raises(ValueError):
        model.infer_batch(unit, g, noise=one, seed=SEED)


# ------------------------------------------------------------------ 7. the memory contract of the new entry points
class RngCase(PathCase):
    """PathCase for the _rng twins: entry = ragged_rng | ragged_rng_fm | fanout_rng | fanout_rng_fm.  No noise tensor
    exists; the key array is an input arena of exactly rows * 8 bytes, so the bytes behind keys_dev[rows - 1] are guard
    (0xFF = NaN patterns under the third fill): a key read past [0, rows) differs between the fills, and so would the
    output."""

    def __init__(self, mc, sd, dtype, unit, g, keys, frames, lens, entry, src=None):
        shape_only = torch.zeros(g.shape[0], mc["inter_channels"], frames)
        super().__init__(mc, sd, dtype, unit, g, shape_only, lens, entry, src)
        self.keys = [k - 2 ** 64 if k >= 2 ** 63 else k for k in keys]
        self.seed, self.scale = SEED, 1.0

    def setup(self, A, poison, lens=None, src=None):
        lens = self.lens if lens is None else lens
        src = self.src if src is None else src
        unit = self.unit.clone()
        for b, n in enumerate(lens):
            unit[b, :, n:] = NAN if poison else 300.0
        if self.entry.endswith("_fm"):
            unit = unit.transpose(1, 2).contiguous()
        t = dict(blob=A.input("blob", self.blob), unit=A.input("unit", unit), g=A.input("g", self.g),
                 keys=A.input("keys_dev", torch.tensor(self.keys, dtype=torch.int64)),
                 ws=A.scratch("workspace", self.n_ws), out=A.output("out", torch.float32, (self.R, 1, self.T * self.spf)),
                 lens=A.input("frames_dev", torch.tensor(lens, dtype=torch.int32)))
        if self.fan:
            t["src"] = A.input("src_of_row_dev", torch.tensor(src, dtype=torch.int32))
        return t

    def invoke(self, t):
        hip, cfgp = self.hip, ctypes.byref(self.cfg)
        p = {k: v.data_ptr() for k, v in t.items()}
        desc = self.L.QvcNoiseRng(self.seed, p["keys"], self.scale)
        if self.fan:
            fn = hip.qvc_infer_fanout_ragged_rng_fm if self.entry.endswith("_fm") else hip.qvc_infer_fanout_ragged_rng
            return fn(cfgp, p["blob"], p["unit"], p["lens"], p["src"], p["g"], ctypes.byref(desc), p["out"], self.U, self.R, self.T,
                      p["ws"], self.n_ws, _stream())
        fn = hip.qvc_infer_batch_ragged_rng_fm if self.entry.endswith("_fm") else hip.qvc_infer_batch_ragged_rng
        return fn(cfgp, p["blob"], p["unit"], p["g"], ctypes.byref(desc), p["out"], self.R, self.T, p["lens"], p["ws"], self.n_ws, _stream())

    def launch_names(self, dev):
        return None                                                     # no timed twin

    def engine_result(self, dev):
        from quickvc_official_amd.engine import QvcEngine
        eng = QvcEngine(self.mc, self.sd, dev)
        unit, g = self.unit.to(dev), self.g.to(dev)
        fm = self.entry.endswith("_fm")
        if fm:
            unit = unit.transpose(1, 2).contiguous()
        rng = (self.seed, self.keys, self.scale)
        if self.fan:
            out = eng.infer_fanout_ragged(unit, _i32(self.lens), _i32(self.src), g, None, unit_fm=fm, rng=rng)
        else:
            out = eng.infer_batch_ragged(unit, g, None, _i32(self.lens), unit_fm=fm, rng=rng)
        torch.cuda.synchronize()
        return out


@pytest.mark.parametrize("entry", ["ragged_rng", "ragged_rng_fm", "fanout_rng", "fanout_rng_fm"])
@pytest.mark.parametrize("name", ["mini", "inter256_h8"])
def test_memory_contract_of_the_rng_entry_points(lib, dev, name, entry):
    """Guards intact, inputs (the key array among them) unchanged, workspace gaps untouched, output identical under the
    three fills (stale workspace is not read; keys_dev is read in [0, rows) only) and equal to the engine's call."""
    _cfg, mc, sd = _problem(name)
    fan = entry.startswith("fanout")
    unit, g = _inputs(name, batch=5 if fan else 2, frames=CS.T, seed0=81)
    if fan:
        case = RngCase(mc, sd, "f16", unit[:2], g, [11, 12, 13, 12, 2 ** 63 + 1], CS.T, list(CS.RAGGED), entry, [1, 0, 1, 0, 1])
    else:
        case = RngCase(mc, sd, "f16", unit, g, [2 ** 64 - 1, 5], CS.T, list(CS.RAGGED), entry)
    got = drive(dev, case.call, locate=lambda fa, fb: case.locate(dev, fa, fb))
    ref = case.engine_result(dev)
    assert torch.equal(got["out"], ref), "the 0x00 run differs from the ordinary engine call"
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0


def test_memory_contract_of_stream_step_rng_and_noise_fill(lib, dev):
    """Every qvc_stream_step_rng of 2 streams (70 and 41 frames, hop 16) to the flush: state zeroed as the header
    requires, everything else from the fill; the noise scratch of the stream workspace is never touched (its bytes keep
    the fill); the concatenated output is identical across fills and equals StreamConverter's.  Then qvc_noise_fill."""
    from quickvc_official_amd import lib as L
    from quickvc_official_amd.streaming import StreamConverter
    _cfg, mc, sd = _problem("mini")
    mcf = dict(mc, operand_dtype="f16")
    cfg = L.make_config(mcf)
    cfgp = ctypes.byref(cfg)
    blob = L.pack_weights(lib, cfg, sd)
    S_, hop, T, lens, keys = 2, 16, 70, [70, 41], [2 ** 33 + 4, 9]
    C = mc["inter_channels"]
    unit, g = _inputs("mini", batch=S_, frames=T, seed0=77)
    n_state, n_ws = int(lib.qvc_stream_state_bytes(cfgp, S_, hop)), int(lib.qvc_stream_workspace_bytes(cfgp, S_, hop))
    lag, nl = int(lib.qvc_stream_lag_frames(cfgp)), int(lib.qvc_stream_noise_lag_frames(cfgp))
    spf = E.samples_per_frame(cfg)
    steps = -(-(T + lag) // hop)
    # Where the pointer form stages its noise: right behind the path workspace of the widest segment (csrc/qvc_stream.h,
    # StreamScratch).  At this config the widest window is enc_p's, hop + 2 * noise_lag frames.  One pointer-form step on
    # a filled workspace shows the region is the right one: that form rewrites all of it.
    noise_off = int(lib.qvc_workspace_bytes(cfgp, S_, hop + 2 * nl))
    noise_len = S_ * C * (2 * nl + hop) * 4
    assert 0 < noise_off and noise_off + noise_len <= n_ws
    probe_ws = torch.full((n_ws + 256,), 0x3C, dtype=torch.uint8, device=dev)
    probe_ws = probe_ws[(-probe_ws.data_ptr()) % 256:][:n_ws]
    probe_state = torch.zeros(n_state + 256, dtype=torch.uint8, device=dev)
    probe_state = probe_state[(-probe_state.data_ptr()) % 256:][:n_state]
    pb, pg = blob.to(dev), g.to(dev)
    pu, pn = torch.zeros(S_, 256, hop, device=dev), torch.ones(S_, C, hop, device=dev)
    po, pp, pl = torch.zeros(S_, hop * spf, device=dev), torch.zeros(S_, dtype=torch.int32, device=dev), _i32(lens).to(dev)
    assert pb.data_ptr() % 256 == 0
    assert lib.qvc_stream_step(cfgp, _ptr(pb), _ptr(probe_state), n_state, _ptr(pu), _ptr(pg), _ptr(pn), _ptr(po), S_, hop, _ptr(pp), _ptr(pl),
                               _ptr(probe_ws), n_ws, _stream()) == 0
    torch.cuda.synchronize()
    region = probe_ws[noise_off:noise_off + noise_len].view(torch.float32).reshape(S_, C, 2 * nl + hop)
    assert float(region[:, :, nl:nl + hop].min()) == 1.0 and float(region[:, :, :nl].abs().max()) == 0.0 and float(region[:, :, nl + hop:].abs().max()) == 0.0

    def call(A, poison):
        bl, gg = A.input("blob", blob), A.input("g", g)
        ln = A.input("len_dev", torch.tensor(lens, dtype=torch.int32))
        kd = A.input("keys_dev", torch.tensor(keys, dtype=torch.int64))
        state = A.scratch("state", n_state)
        state.zero_()
        ws, out = A.scratch("workspace", n_ws), A.output("out", torch.float32, (S_, hop * spf))
        desc = L.QvcNoiseRng(SEED, _ptr(kd), 1.0)
        whole = torch.zeros(S_, 1, T * spf, device=dev)
        status = 0
        for n in range(steps):
            s = n * hop
            u_new = torch.full((S_, 256, hop), NAN if poison else 123.0)
            for b, end in enumerate(lens):
                lo, hi = s, min(s + hop, end)
                if hi > lo:
                    u_new[b, :, :hi - lo] = unit[b, :, lo:hi]
            ud = A.input("unit_new", u_new)
            pos = A.input("pos_dev", torch.full((S_,), s, dtype=torch.int32))
            out.view(torch.uint8).fill_(A.fill)
            st = lib.qvc_stream_step_rng(cfgp, _ptr(bl), _ptr(state), n_state, _ptr(ud), _ptr(gg), ctypes.byref(desc), _ptr(out), S_, hop,
                                         _ptr(pos), _ptr(ln), _ptr(ws), n_ws, _stream())
            status = status or st
            f0 = s - lag
            lo, hi = max(f0, 0), min(f0 + hop, T)
            if hi > lo:
                whole[:, 0, lo * spf:hi * spf] = out[:, (lo - f0) * spf:(hi - f0) * spf]
            if f0 + hop <= 0 or f0 >= T:
                assert float(out.abs().max()) == 0.0, n
        # "never touches the X.noise scratch": every byte of it still holds the fill
        assert bool((ws[noise_off:noise_off + noise_len] == A.fill).all())
        return dict(status=status, outs=dict(whole=whole), zero=[whole[b, :, end * spf:] for b, end in enumerate(lens)])

    got = drive(dev, call)
    model = _mini_model(dev)
    conv = StreamConverter(model, streams=S_, hop_frames=hop, use_graph=False, seed=SEED)
    ref = conv.convert(unit.to(dev), g.to(dev), lengths=_i32(lens), seed=SEED, keys=keys)
    torch.cuda.synchronize()
    assert torch.equal(got["whole"], ref) and bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0

    def fill_call(A, poison):
        kd = A.input("keys_dev", torch.tensor([7, -3, 0x100000002], dtype=torch.int64))
        out = A.output("noise_out", torch.float32, (3, 32, 64))
        st = lib.qvc_noise_fill(SEED, _ptr(kd), 1.0, 3, 32, 64, 5, _ptr(out), _stream())
        return dict(status=st, outs=dict(noise=out))
    filled = drive(dev, fill_call)
    want = NH.noise_tensor(SEED, [7, 2 ** 64 - 3, 0x100000002], 32, 64, frame0=5)
    assert float(np.abs(filled["noise"].cpu().numpy().astype(np.float64) - want).max()) <= 1.5e-5


# ------------------------------------------------------------------ 8. the oracle
@pytest.mark.parametrize("dtype,min_db", [("f16", 50.0), ("bf16x", 40.0)])
def test_rng_conversion_against_the_oracle(lib, dev, dtype, min_db):
    """The fp32 oracle fed the tensor qvc_noise_fill wrote, against the rng conversion, per batch member."""
    cfg, _mc, sd = _problem("mini")
    eng = _engine("mini", dev, dtype)
    unit, g = _inputs("mini")
    keys = [3, 4]
    noise = eng.noise_fill(SEED, keys, cfg["inter_channels"], CS.T).cpu()
    out = eng.infer_batch_ragged(unit.to(dev), g.to(dev), None, _i32([CS.T, CS.T]), rng=(SEED, keys, 1.0)).cpu()
    ref = oracle.infer_from_g(sd, cfg, unit, g.unsqueeze(-1), noise)
    for b in range(CS.B):
        db = snr_db(ref[b], out[b])
        print(f"{dtype} member {b}: {db:.1f} dB against the oracle")
        assert db >= min_db, (dtype, b, db)


# ------------------------------------------------------------------ 9. the CLI
def test_convert_cli_native_noise_does_not_depend_on_the_batching(lib, dev, tmp_path):
    """A 9-line list (6 unit files, three of them listed twice; 2 targets) through the CLI with --noise native at --batch 4
    and --batch 7 without fan-out and at --batch 7 with it: the wav files are byte-identical across the three runs, and a
    line converted alone under its list index as key gives the same samples.  --noise torch (the default) still writes
    what batch_noise and the pointer entry points give for the run's own batches -- the parent's pipeline, recomputed
    here batch by batch."""
    from scipy.io import wavfile
    import quickvc_official_amd as q
    from quickvc_official_amd import convert as cli
    from quickvc_official_amd.checkpoint import save_checkpoint
    from quickvc_official_amd.frontend import MelFrontend, load_wav
    from quickvc_official_amd.synth import make_synthetic_state_dict
    cfg = {"train": {"segment_size": 10240}, "data": dict(q.DEFAULT_DATA_CONFIG), "model": dict(q.MINI_MODEL_CONFIG)}
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    model = q.SynthesizerTrn(641, 32, **q.MINI_MODEL_CONFIG)
    model.load_state_dict(make_synthetic_state_dict(model, 21))
    save_checkpoint(model, None, 2e-4, 1, str(tmp_path / "G_1.pth"))
    sr = cfg["data"]["sampling_rate"]
    t = np.arange(int(1.5 * sr)) / sr
    for k in range(2):
        wavfile.write(str(tmp_path / f"spk{k}.wav"), sr, (0.4 * np.sin(2 * np.pi * (140.0 + 45.0 * k) * t) * 32767).astype(np.int16))
    rs = np.random.RandomState(41)
    src_len = [31, 24, 40, 27, 35, 22]
    for i, n in enumerate(src_len):
        np.save(str(tmp_path / f"u{i}.npy"), rs.randn(n, 256).astype(np.float32))
    lines = [0, 1, 2, 0, 3, 4, 2, 5, 4]                                 # sources 0, 2, 4 twice, to the other target
    items = [(f"o{k}", str(tmp_path / f"u{s}.npy"), str(tmp_path / f"spk{(k // 3) % 2}.wav")) for k, s in enumerate(lines)]
    (tmp_path / "convert.txt").write_text("".join(f"{a}|{b}|{c}\n" for a, b, c in items))
    base = ["--hpfile", str(tmp_path / "config.json"), "--ptfile", str(tmp_path / "G_1.pth"), "--txtpath", str(tmp_path / "convert.txt"),
            "--seed", "5", "--io-threads", "2"]
    runs = {"b4": ["--batch", "4", "--fanout", "off"], "b7": ["--batch", "7", "--fanout", "off"], "fan": ["--batch", "7"]}
    for tag, extra in runs.items():
        stats = cli.main(base + ["--noise", "native", "--outdir", str(tmp_path / tag)] + extra)
        assert stats["utterances"] == 9, (tag, stats)
        assert (stats["encodes_saved"] > 0) == (tag == "fan"), (tag, stats)
    for k in range(9):
        raw = [open(str(tmp_path / tag / f"o{k}.wav"), "rb").read() for tag in runs]
        assert raw[0] == raw[1] == raw[2], k
    # a line alone, keyed by its list index (taken before sharding and length-sorting)
    net = q.SynthesizerTrn(641, 32, **q.MINI_MODEL_CONFIG).cuda().eval()
    q.load_checkpoint(str(tmp_path / "G_1.pth"), net, None)
    d = cfg["data"]
    front = MelFrontend(d["filter_length"], d["n_mel_channels"], sr, d["hop_length"], d["win_length"], d["mel_fmin"], d["mel_fmax"])
    tgts = [str(tmp_path / "spk0.wav"), str(tmp_path / "spk1.wav")]
    table = net.speaker_embed_waves([load_wav(p, sr) for p in tgts], front, trim_top_db=20)      # as the CLI embeds them: one chunk
    g_of = lambda k: table[(k // 3) % 2].unsqueeze(0)
    for k in (0, 4, 8):
        unit = torch.from_numpy(np.load(items[k][1])).t().unsqueeze(0).cuda()
        alone = net.infer_batch(unit, g_of(k), seed=5, keys=[k])
        _r, w = wavfile.read(str(tmp_path / "b4" / f"o{k}.wav"))
        assert np.array_equal(alone[0, 0].cpu().numpy(), w), (k, snr_db(alone[0, 0].cpu().numpy(), w))
    # scale 0: the mean conversion, the same whatever the seed
    cli.main(base + ["--noise", "native", "--noise-scale", "0", "--batch", "4", "--outdir", str(tmp_path / "mean5")])
    cli.main(base[:-4] + ["--seed", "6", "--io-threads", "2", "--noise", "native", "--noise-scale", "0", "--batch", "4", "--outdir", str(tmp_path / "mean6")])
    assert open(str(tmp_path / "mean5" / "o3.wav"), "rb").read() == open(str(tmp_path / "mean6" / "o3.wav"), "rb").read()
    assert open(str(tmp_path / "mean5" / "o3.wav"), "rb").read() != open(str(tmp_path / "b4" / "o3.wav"), "rb").read()
    # --noise torch: the parent's pipeline, batch by batch
    stats = cli.main(base + ["--batch", "4", "--outdir", str(tmp_path / "torch")])
    assert stats["utterances"] == 9
    lengths, _mine, batches = cli.rank_plan(items, 0, 1, 4)
    eng = net.engine()
    inter = q.MINI_MODEL_CONFIG["inter_channels"]
    for idxs in batches:
        n, tmax = len(idxs), max(lengths[i] for i in idxs)
        uniq, src_of_row = cli.fanout_rows([items[i][1] for i in idxs])
        unit = torch.zeros(len(uniq), tmax, 256)
        for u, p in enumerate(uniq):
            a = np.load(p)
            unit[u, :len(a)] = torch.from_numpy(a)
        ulens = _i32([len(np.load(p)) for p in uniq])
        noise = cli.batch_noise(5, idxs[0], n, inter, tmax, dev)
        g = torch.cat([g_of(i) for i in idxs])
        if len(uniq) < n:
            out = eng.infer_fanout_ragged(unit.to(dev), ulens, _i32(src_of_row), g, noise, unit_fm=True)
        else:
            out = eng.infer_batch_ragged(unit.to(dev), g, noise, ulens, unit_fm=True)
        torch.cuda.synchronize()
        for r, i in enumerate(idxs):
            _r, w = wavfile.read(str(tmp_path / "torch" / f"o{i}.wav"))
            assert np.array_equal(out[r, 0, :lengths[i] * 320].cpu().numpy(), w), i
    with pytest.raises(SystemExit):
        cli.main(base + ["--noise-scale", "0.5", "--outdir", str(tmp_path / "bad")])
