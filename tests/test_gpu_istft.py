"""GPU tests of the single-band iSTFT decoder (istft_vits=True, iSTFT_Generator models.py:98-192) on an MI355X.

Tolerances are the ones tests/test_gpu_parity.py states: waveform SNR per utterance against the reference's goldens
f16 >= 45 dB and bf16x >= 40 dB; the fp32 tail >= 100 dB against the fp64 closed form; launch variants bit-identical.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import istft_ref
from helpers import GOLDEN, regenerate, snr_db

pytestmark = pytest.mark.gpu

DEBUG_DEFAULTS = {"post_tail": 1, "post_tail_nf": 4, "pair_wide_launch": 1, "pair_cm4": 1, "conv_cl": 1, "wn_chunk": 0,
                  "pair_chain3": 0, "wn_kernel": 0, "launch_stop": -1}
BARS = {"f16": 45.0, "bf16x": 40.0}


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


def load_istft_case(name):
    with open(os.path.join(GOLDEN, "istft_manifest.json")) as f:
        entry = json.load(f)[name]
    return entry, dict(np.load(os.path.join(GOLDEN, entry["file"])))


def _engine(mc, sd, dev, dtype):
    import quickvc_official_amd as q
    from quickvc_official_amd.engine import QvcEngine
    model = q.SynthesizerTrn(641, 32, **mc)
    return QvcEngine(dict(model.model_config, operand_dtype=dtype), sd, dev)


@pytest.mark.parametrize("name", ["istft_mini", "istft_full_b1", "istft_ups3"])
def test_single_band_path_matches_reference_goldens(lib, dev, name):
    """SynthesizerTrn(istft_vits=True).infer_batch on the HIP path against the waveform recorded from the reference's
    iSTFT_Generator (320 samples per unit frame)."""
    import quickvc_official_amd as q
    entry, arrays = load_istft_case(name)
    _m, sd, unit, g, noise = regenerate(entry)
    ref = torch.from_numpy(arrays["o"]).reshape(tuple(arrays["o::shape"]))
    assert ref.shape[-1] == 320 * entry["frames"]
    for dt, bar in BARS.items():
        model = q.SynthesizerTrn(641, 32, **entry["config"], operand_dtype=dt)
        model.load_state_dict(sd)
        model = model.to(dev).eval()
        out = model.infer_batch(unit.to(dev), g.to(dev), noise.to(dev)).cpu()
        assert out.shape == ref.shape
        for b in range(ref.shape[0]):
            s = snr_db(ref[b], out[b])
            assert s >= bar, (name, dt, b, s)


@pytest.mark.parametrize("which", ["ups3", "odd"])
def test_single_band_other_geometries_match_restatement(lib, dev, which):
    """A three-up-sampler geometry ([8, 5, 2] / [16, 9, 4]) and widths that are not multiples of the MFMA K step
    against the test-side restatement (fp32 on the CPU)."""
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_state_dict, make_synthetic_inputs
    base = dict(q.ISTFT_MODEL_CONFIG) if which == "ups3" else dict(q.ODD_MODEL_CONFIG, ms_istft_vits=False, istft_vits=True,
                                                                       upsample_rates=[10, 8], upsample_kernel_sizes=[20, 16])
    if which == "ups3":
        base.update(upsample_rates=[8, 5, 2], upsample_kernel_sizes=[16, 9, 4], inter_channels=64, hidden_channels=64,
                    upsample_initial_channel=128, gin_channels=64)
    model = q.SynthesizerTrn(641, 32, **base)
    sd = make_synthetic_state_dict(model, 77)
    unit, g, noise = make_synthetic_inputs(2, 33, 256, base["inter_channels"], base["gin_channels"], seed0=9)
    ref = istft_ref.infer_from_g_single(sd, base, unit, g.unsqueeze(-1), noise)
    for dt, bar in BARS.items():
        eng = _engine(base, sd, dev, dt)
        out = eng.infer_batch(unit.to(dev), g.to(dev), noise.to(dev)).cpu()
        assert out.shape == ref.shape == (2, 1, 320 * 33)
        for b in range(2):
            assert snr_db(ref[b], out[b]) >= bar, (which, dt, b, snr_db(ref[b], out[b]))


def test_single_band_istft_synth_matches_closed_form(lib, dev):
    """qvc_istft_synth for the single-band decoder (fp32 post-conv frames -> waveform) against the fp64 closed form;
    y_mb receives the one band signal, which is the waveform itself."""
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_state_dict
    model = q.SynthesizerTrn(641, 32, **q.ISTFT_MODEL_CONFIG)
    eng = _engine(q.ISTFT_MODEL_CONFIG, make_synthetic_state_dict(model, 5), dev, "f16")
    gen = torch.Generator().manual_seed(3)
    for F_ in (2, 5, 257, 1201):
        post = torch.randn(3, F_, 18, generator=gen) * 0.7
        out, ymb = eng.istft_synth(post.to(dev), want_bands=True)
        out, ymb = out.cpu(), ymb.cpu()
        ref = istft_ref.post_frames_to_wave(post)
        assert out.shape == ref.shape == (3, 1, 4 * (F_ - 1)) and ymb.shape == (3, 1, 4 * (F_ - 1))
        for b in range(3):
            assert snr_db(ref[b], out[b]) >= 100.0, (F_, b)
        assert torch.equal(ymb, out)


def test_single_band_fused_tail_is_bit_identical_to_two_launches(lib, dev):
    """conv_post + single-band tail as one launch (post_tail_kernel<T, 2, 1>) against the debug switch post_tail = 0
    (conv_post -> fp32 frames -> istft_synth_kernel<1>): bit-identical, for a whole and a ragged batch.  The timed
    records show exactly one fused single-band tail launch and no standalone tail (or the reverse)."""
    import quickvc_official_amd as q
    from quickvc_official_amd import lib as L
    from quickvc_official_amd.synth import make_synthetic_state_dict, make_synthetic_inputs
    mc = q.ISTFT_MODEL_CONFIG
    sd = make_synthetic_state_dict(q.SynthesizerTrn(641, 32, **mc), 1234)
    unit, g, noise = make_synthetic_inputs(2, 130, 256, 192, 256, seed0=11)
    lens = torch.tensor([130, 77], dtype=torch.int32)
    outs = {}
    for fused in (1, 0):
        L.debug_set("post_tail", fused)
        for dt in ("f16", "bf16x"):
            eng = _engine(mc, sd, dev, dt)
            out, recs = eng.infer_batch_timed(unit.to(dev), g.to(dev), noise.to(dev))
            torch.cuda.synchronize()
            names = [r["name"] for r in recs]
            n_fused = sum(n.startswith("post_tail1<") for n in names)
            n_tail = sum(n == "istft1" for n in names)
            assert (n_fused, n_tail) == ((1, 0) if fused else (0, 1)), names
            assert not any(n.startswith("post_tail<") or n == "istft_synth" for n in names), names
            rag = eng.infer_batch_ragged(unit.to(dev), g.to(dev), noise.to(dev), lens.to(dev))
            plain = eng.infer_batch(unit.to(dev), g.to(dev), noise.to(dev))
            torch.cuda.synchronize()
            outs[(fused, dt)] = (plain.cpu(), rag.cpu())
    for dt in ("f16", "bf16x"):
        assert torch.equal(outs[(1, dt)][0], outs[(0, dt)][0]), dt
        assert torch.equal(outs[(1, dt)][1], outs[(0, dt)][1]), dt


def test_single_band_ragged_batch(lib, dev):
    """A ragged batch: the full-length member equals the plain batch, the short one equals itself converted alone,
    and every row is zero past its own length."""
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_state_dict, make_synthetic_inputs
    mc = q.ISTFT_MODEL_CONFIG
    sd = make_synthetic_state_dict(q.SynthesizerTrn(641, 32, **mc), 4)
    unit, g, noise = make_synthetic_inputs(3, 90, 256, 192, 256, seed0=21)
    lens = torch.tensor([90, 41, 3], dtype=torch.int32)
    eng = _engine(mc, sd, dev, "f16")
    rag = eng.infer_batch_ragged(unit.to(dev), g.to(dev), noise.to(dev), lens.to(dev)).cpu()
    plain = eng.infer_batch(unit.to(dev), g.to(dev), noise.to(dev)).cpu()
    assert torch.equal(rag[0], plain[0])
    for b, n in enumerate(lens.tolist()):
        assert rag[b, 0, 320 * n:].abs().max() == 0 if n < 90 else True
        assert rag[b, 0, :320 * n].abs().max() > 0
        alone = eng.infer_batch(unit[b:b + 1, :, :n].contiguous().to(dev), g[b:b + 1].to(dev),
                                noise[b:b + 1, :, :n].contiguous().to(dev)).cpu()
        assert snr_db(alone[0, 0], rag[b, 0, :320 * n]) >= 100.0, b


def test_single_band_convert_cli(lib, dev, tmp_path):
    """python -m quickvc_official_amd.convert surface with a config JSON that sets istft_vits: files to files,
    320 samples per unit frame, equal to what the Python API computes from the same files and seed."""
    from scipy.io import wavfile
    import quickvc_official_amd as q
    from quickvc_official_amd import convert as cli
    from quickvc_official_amd.checkpoint import save_checkpoint
    from quickvc_official_amd.frontend import MelFrontend, load_wav, trim
    from quickvc_official_amd.synth import make_synthetic_state_dict
    mc = dict(q.MINI_MODEL_CONFIG, ms_istft_vits=False, istft_vits=True, upsample_rates=[10, 8], upsample_kernel_sizes=[20, 16])
    cfg = {"train": {"segment_size": 10240}, "data": dict(q.DEFAULT_DATA_CONFIG), "model": mc}
    hp = tmp_path / "config.json"
    hp.write_text(json.dumps(cfg))
    model = q.SynthesizerTrn(641, 32, **mc)
    model.load_state_dict(make_synthetic_state_dict(model, 21))
    pt = tmp_path / "G_1.pth"
    save_checkpoint(model, None, 2e-4, 1, str(pt))
    sr = cfg["data"]["sampling_rate"]
    t = np.arange(int(1.7 * sr)) / sr
    tgt = (0.4 * np.sin(2 * np.pi * 180 * t) * (t > 0.2) * (t < 1.5)).astype(np.float32)
    wavfile.write(str(tmp_path / "tgt.wav"), sr, (tgt * 32767).astype(np.int16))
    rng = np.random.RandomState(5)
    for name, frames in (("a", 81), ("b", 81), ("c", 40)):
        np.save(str(tmp_path / f"{name}.npy"), rng.randn(frames, 256).astype(np.float32))
    (tmp_path / "convert.txt").write_text("".join(f"t_{n}|{tmp_path}/{n}.npy|{tmp_path}/tgt.wav\n" for n in "abc"))
    out = tmp_path / "out"
    cli.main(["--hpfile", str(hp), "--ptfile", str(pt), "--txtpath", str(tmp_path / "convert.txt"), "--outdir", str(out),
              "--seed", "7", "--batch", "2"])
    d = cfg["data"]
    wav = torch.from_numpy(trim(load_wav(str(tmp_path / "tgt.wav"), sr), top_db=20)).unsqueeze(0)
    mel = MelFrontend(d["filter_length"], d["n_mel_channels"], sr, d["hop_length"], d["win_length"], d["mel_fmin"], d["mel_fmax"])(wav)
    net = model.cuda().eval()
    g = net.speaker_embed(mel)
    inter = mc["inter_channels"]
    n_ab = cli.batch_noise(7, 0, 2, inter, 81, dev)
    noises = {"a": n_ab[0], "b": n_ab[1], "c": cli.batch_noise(7, 2, 1, inter, 40, dev)[0]}
    for name, frames in (("a", 81), ("b", 81), ("c", 40)):
        rate, got = wavfile.read(str(out / f"t_{name}.wav"))
        assert rate == sr and got.dtype == np.float32 and got.shape == (320 * frames,)
        assert np.isfinite(got).all() and np.abs(got).max() > 0
        unit = torch.from_numpy(np.load(str(tmp_path / f"{name}.npy"))).t()[None].cuda()
        ref = net.infer_batch(unit, g, noises[name][None])
        assert snr_db(ref[0, 0].cpu().numpy(), got) >= 100.0, name


def test_single_band_streaming_is_refused(lib, dev):
    import quickvc_official_amd as q
    from quickvc_official_amd import lib as L
    from quickvc_official_amd.streaming import StreamConverter
    from quickvc_official_amd.synth import make_synthetic_state_dict
    model = q.SynthesizerTrn(641, 32, **q.ISTFT_MODEL_CONFIG)
    model.load_state_dict(make_synthetic_state_dict(model, 2))
    model = model.to(dev).eval()
    with pytest.raises(L.QvcError):
        StreamConverter(model, 2, 20)
