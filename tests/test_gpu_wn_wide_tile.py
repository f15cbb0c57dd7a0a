"""GPU test of the 64-frame WaveNet stack tile (qvc_wn2_impl.h, NF = 5) against the 32-frame tile of the same kernel:
same K order per output, same roundings -> bit-identical.  The tiles are forced with the library's debug switch
wn_kernel (2 = 32-frame, 3 = 64-frame), which is put back in a `finally`.  Covered: enc_p and the four coupling
stacks (pre / post fused), f16 and bf16, T = 250 and an odd T = 37, a ragged batch, batch 1 and batch 32; and the
default selection (the 64-frame tile where the 32-frame grid fills the chip, the 32-frame tile at batch 1)."""
import pytest
import torch

from helpers import load_case, regenerate

pytestmark = pytest.mark.gpu


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


@pytest.fixture(scope="module")
def model():
    entry, _ = load_case("full_b1")
    _m, sd, _u, _g, _n = regenerate(entry)
    return entry, sd


def _engine(entry, sd, dev, dtype):
    import quickvc_official_amd as q
    from quickvc_official_amd.engine import QvcEngine
    m = q.SynthesizerTrn(641, 32, **entry["config"])
    return QvcEngine(dict(m.model_config, operand_dtype=dtype), sd, dev)


def _run(eng, dev, B, T, seed):
    from quickvc_official_amd.synth import make_synthetic_inputs
    unit, g, noise = make_synthetic_inputs(B, T, 256, 192, 256, seed0=seed)
    z = eng.enc_p(unit, noise)
    zf = eng.flow_reverse(z, g)
    gen = torch.Generator(device=dev).manual_seed(seed)
    ws = [eng.wn_stack(i, torch.randn(B, T, 192, device=dev, generator=gen), g) for i in range(5)]
    out, recs = eng.infer_batch_timed(unit.to(dev), g.to(dev), noise.to(dev))
    res = [z, zf, out, *ws]
    if B > 1:
        lens = torch.randint(1, T + 1, (B,), generator=torch.Generator().manual_seed(seed)).to(torch.int32)
        lens[0] = T
        res.append(eng.infer_batch_ragged(unit.to(dev), g.to(dev), noise.to(dev), lens.to(dev)))
    torch.cuda.synchronize()
    names = [r["name"] for r in recs if r["name"].startswith("wn_stack")]
    return [t.cpu() for t in res], names


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("B,T", [(32, 250), (1, 250), (5, 37), (1, 37)])
def test_wide_wn_tile_is_bit_identical_to_32_frame_tile(lib, dev, model, dtype, B, T):
    from quickvc_official_amd import lib as L
    entry, sd = model
    eng = _engine(entry, sd, dev, dtype)
    res = {}
    try:
        for variant in (2, 3):
            L.debug_set("wn_kernel", variant)
            res[variant] = _run(eng, dev, B, T, seed=5100 + B + T)
    finally:
        L.debug_set("wn_kernel", 0)
    (a, na), (b, nb) = res[2], res[3]
    assert len(na) == 8 and not any(n.endswith(",64f>") for n in na), na
    assert len(nb) == 8 and all(n.startswith("wn_stack2<") and n.endswith(",64f>") for n in nb), nb
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (dtype, B, T, i, (x - y).abs().max().item())


def test_default_selection_of_the_wn_tile(lib, dev, model):
    from quickvc_official_amd import lib as L
    entry, sd = model
    assert L.debug_get("wn_kernel") == 0
    eng = _engine(entry, sd, dev, "f16")
    _, big = _run(eng, dev, 32, 250, seed=77)
    _, one = _run(eng, dev, 1, 250, seed=78)
    assert len(big) == 8 and all(n.endswith(",64f>") for n in big), big
    assert len(one) == 8 and all(n.startswith("wn_stack2<") and not n.endswith(",64f>") for n in one), one
