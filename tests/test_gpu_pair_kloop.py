"""The K loop of the fused ResBlock pair kernel at every trip count it treats differently (run with -m gpu).

The loop runs whole groups of four k-steps with no test around a load and a guarded remainder of nIt % 4 steps
(all of them when nIt < 4).  The shipped shapes have nIt in {12, 28, 44, 24, 56, 88}: no remainder, so nothing in
the rest of the suite walks the remainder or a ring that is never full.  Here the generator trunk (qvc_dec_trunk)
runs on small configs whose pair convs have nIt = taps * ceil(channels / 32) =
    1, 2 (shorter than the ring), 3, 5, 6, 7 (every remainder, with and without whole groups before it), 10, 14,
    and 4, 12, 28 (whole groups only),
in the f16 and bf16x modes, against the CPU oracle, and a ragged batch of two (the second utterance ends inside a
tile at both stages) against that utterance converted alone.

Shapes: T = 40 frames, batch 2.  Channel counts 16-48 with ResBlock kernels 3 / 5 / 7 alone cannot give every count
asked for -- nIt is then k or 2k with k odd: never 1, 2 or a multiple of four -- so kernel size 1 (nIt 1 and 2) and
one config with 128 / 64 channels (nIt 4, 12, 28) are added to them.

Tolerances, as tests/test_gpu_parity.py has them for stage-level parity (the stage fed with the input the oracle's
stage gets; here a unit-variance latent): 5 dB above the whole-path bar of the mode -- f16 45 + 5 = 50 dB, bf16x
40 + 5 = 45 dB; ragged member against the utterance alone >= 100 dB (the project's bar for launch-shape variants).
"""
import ctypes

import pytest
import torch

import qvc_oracle as oracle
from helpers import snr_db

pytestmark = pytest.mark.gpu

T, B, SHORT = 40, 2, 23

CONFIGS = {
    # name: (upsample_initial_channel, resblock kernel sizes) -> stage channels init/2, init/4
    "c48_c24_k135": (96, [1, 3, 5]),      # 48 channels: nIt 2, 6, 10;  24 channels: 1, 3, 5
    "c32_c16_k357": (64, [3, 5, 7]),      # 32 and 16 channels: 3, 5, 7
    "c128_c64_k137": (256, [1, 3, 7]),    # 128 channels: 4, 12, 28;  64 channels: 2, 6, 14
}
STAGE_DB = {"f16": 50.0, "bf16x": 45.0}


def _n_it(init, kernels):
    """ConvDesc::nIt of the pair convs of both stages: taps * (channels padded to 32) / 32."""
    return {k * -(-ch // 32) for ch in (init // 2, init // 4) for k in kernels}


def test_the_configs_cover_every_trip_count():
    seen = set().union(*(_n_it(*c) for c in CONFIGS.values()))
    assert {1, 2, 3, 5, 6, 7} <= seen, seen
    assert any(n % 4 == 0 for n in seen), seen
    assert any(n > 4 and n % 4 for n in seen), seen               # whole groups AND a remainder


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


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def case(request):
    """Model, inputs and the oracle's taps of one config: computed once, shared by the modes, left unchanged."""
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_state_dict, make_synthetic_inputs
    init, kernels = CONFIGS[request.param]
    cfg = dict(q.MINI_MODEL_CONFIG, upsample_initial_channel=init, resblock_kernel_sizes=kernels)
    model = q.SynthesizerTrn(641, 32, **cfg)
    sd = make_synthetic_state_dict(model, 4100 + init)
    unit, g, noise = make_synthetic_inputs(B, T, 256, cfg["inter_channels"], cfg["gin_channels"], seed0=23 + init)
    # the trunk alone, fed with a unit-variance latent (the noise tensor): the encoder and the flow are not under test
    taps = {}
    with torch.no_grad():
        oracle.decoder_forward({k: v.float() for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()},
                               cfg, noise, g.unsqueeze(-1), taps)
    z = noise.transpose(1, 2).contiguous()
    want = taps["dec.subband_conv_post"].transpose(1, 2).contiguous()
    return request.param, model.model_config, sd, unit, g, noise, z, want


@pytest.mark.parametrize("dtype", ["f16", "bf16x"])
def test_trunk_parity_and_ragged_member_through_the_pair_kernel(lib, dev, case, dtype):
    from quickvc_official_amd.engine import QvcEngine
    name, mc, sd, unit, g, noise, z, want = case
    eng = QvcEngine(dict(mc, operand_dtype=dtype), sd, dev)
    info = (ctypes.c_int32 * 8)()
    assert lib.qvc_plan_info(ctypes.byref(eng.cfg), info) == 0 and info[7] == 1, list(info)      # every pair fusable
    # ... and launched as pairs: at this size the three chains of a stage share one launch per pair, none is chained
    _out, recs = eng.infer_batch_timed(unit.to(dev), g.to(dev), noise.to(dev))
    names = [r["name"] for r in recs]
    assert sum(n.startswith("rbpair<") for n in names) == 6 and not any(n.startswith("rbchain<") for n in names), names

    post = eng.dec_trunk(z, g)
    torch.cuda.synchronize()
    db = snr_db(want, post.cpu())
    print(f"{name} {dtype}: trunk vs oracle {db:.1f} dB")
    assert bool(torch.isfinite(post).all()) and db >= STAGE_DB[dtype], (name, dtype, db)

    lens = [T, SHORT]
    pad_u, pad_n = unit.clone(), noise.clone()
    pad_u[1, :, SHORT:] = 300.0                                     # junk the path must never read unmasked
    pad_n[1, :, SHORT:] = float("nan")
    rag = eng.infer_batch_ragged(pad_u.to(dev), g.to(dev), pad_n.to(dev), torch.tensor(lens, dtype=torch.int32)).clone()
    alone = eng.infer_batch(unit[1:2, :, :SHORT].to(dev), g[1:2].to(dev), noise[1:2, :, :SHORT].to(dev))
    torch.cuda.synchronize()
    spf = eng.samples_per_frame
    db = snr_db(alone[0].cpu(), rag[1, :, :spf * SHORT].cpu())
    print(f"{name} {dtype}: ragged member vs alone {db:.1f} dB")
    assert bool(torch.isfinite(rag).all()) and db >= 100.0, (name, dtype, db)
    assert float(rag[1, :, spf * SHORT:].abs().max()) == 0.0
