"""GPU tests (-m gpu) of the target recordings' native route and of 16-bit output: raw wav payloads decoded on the device
(qvc_pcm_to_wave_ragged), speaker embeddings from files (SynthesizerTrn.speaker_embed_files), fp32 -> int16
(qvc_wave_to_pcm16) and the CLI flags --target-io / --pcm16.

The contract is equality, not a tolerance: a decoded row is frontend.load_wav of its file bit for bit (the arithmetic is
load_wav's: a power-of-two scale after an exact or round-to-nearest-even int -> float conversion, and (a + b) * 0.5f for two
channels), so the embeddings of the two routes are equal and the output files byte-identical; the 16-bit conversion is
the numpy expression of include/qvc.h, NaN -> 0."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import wavgen
from memguard import ArenaSet, describe_guards

pytestmark = pytest.mark.gpu

SR = 16000
LENGTHS = [0, 1, 5, 1023, 1024, 1025, 4099]      # empty, shorter than one vector access, around a 1024 boundary, an odd s24 byte count
MAX_SAMPLES = 4100


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


@pytest.fixture(scope="module")
def pool():
    from quickvc_official_amd import fileio
    p = fileio.IoPool(4)
    yield p
    p.close()


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """{(fmt, channels): [(path, load_wav reference)] for LENGTHS}: written and decoded on the host once."""
    from quickvc_official_amd.frontend import load_wav
    d = tmp_path_factory.mktemp("wavs")
    out = {}
    for fi, fmt in enumerate(wavgen.FORMATS):
        for ch in (1, 2):
            rows = []
            for li, n in enumerate(LENGTHS):
                p = str(d / f"{fmt}_{ch}_{n}.wav")
                wavgen.write_wav(p, fmt, n, ch, seed=100 * fi + 10 * ch + li, rate=SR, extensible=bool(li & 1),
                                 extra=("none", "before", "after")[li % 3])
                if n:
                    ref = load_wav(p, SR)
                else:                                                     # scipy's empty array has no channel axis to average
                    ref = np.zeros(0, dtype=np.float32)
                assert ref.dtype == np.float32 and ref.shape == (n,)
                rows.append((p, ref))
            out[(fmt, ch)] = rows
    return out


def _stage(pool, paths, dev):
    """Payloads of `paths` in 16-byte-multiple slots + their row table, on the device."""
    hdr, st = pool.wav_headers(paths)
    assert st == [0] * len(paths)
    need = max(max(h.frames * h.channels * (h.bits // 8) for h in hdr), 1)
    slot = -(-need // 16) * 16
    host = torch.full((len(paths) * slot,), 0xEE, dtype=torch.uint8)
    hdr2, st2 = pool.load_wavs(paths, host, slot)
    assert st2 == [0] * len(paths)
    rows = torch.tensor([[h.code, h.channels, h.frames] for h in hdr2], dtype=torch.int32)
    return host.to(dev), slot, rows.to(dev)


def _padded(refs, max_samples):
    want = torch.zeros(len(refs), max_samples)
    for u, r in enumerate(refs):
        want[u, :len(r)] = torch.from_numpy(r)
    return want


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("fmt", wavgen.FORMATS)
def test_decode_equals_load_wav(lib, dev, pool, corpus, fmt, channels):
    from quickvc_official_amd.frontend import pcm_to_wave
    rows = corpus[(fmt, channels)]
    pcm, slot, table = _stage(pool, [p for p, _ in rows], dev)
    wave, samples = pcm_to_wave(pcm, slot, table, MAX_SAMPLES)
    assert wave.shape == (len(rows), MAX_SAMPLES) and samples.tolist() == LENGTHS
    want = _padded([r for _, r in rows], MAX_SAMPLES)
    for u in range(len(rows)):
        assert torch.equal(wave[u].cpu(), want[u]), (fmt, channels, LENGTHS[u])
    # a width that is no multiple of four (rows start unaligned: the scalar stores) cuts the longest row and nothing else
    wave2, samples2 = pcm_to_wave(pcm, slot, table, 4097)
    assert samples2.tolist() == [min(n, 4097) for n in LENGTHS]
    assert torch.equal(wave2.cpu(), want[:, :4097])


def _mixed(corpus):
    picks = [("u8", 1, 1023), ("s16", 2, 4099), ("s24", 1, 1025), ("f32", 2, 5), ("s32", 1, 4099), ("u8", 2, 1), ("s24", 2, 4099),
             ("s16", 1, 1024), ("f32", 1, 0), ("s32", 2, 1025)]
    return [corpus[(f, c)][LENGTHS.index(n)] for f, c, n in picks], [n for _, _, n in picks]


def test_decode_mixed_formats_in_a_guarded_arena(lib, dev, pool, corpus):
    rows, lens = _mixed(corpus)
    pcm, slot, table = _stage(pool, [p for p, _ in rows], dev)
    U = len(rows)
    ar = ArenaSet(dev, 0xFF, 0xFF)
    pcm_a = ar.input("pcm", pcm.cpu())
    table_a = ar.input("rows", table.cpu())
    wave = ar.output("wave", torch.float32, (U, MAX_SAMPLES))
    samples = ar.output("samples", torch.int32, (U,))
    st = lib.qvc_pcm_to_wave_ragged(pcm_a.data_ptr(), slot, table_a.data_ptr(), wave.data_ptr(), samples.data_ptr(), U, MAX_SAMPLES,
                                    torch.cuda.current_stream(dev).cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    assert samples.tolist() == lens
    want = _padded([r for _, r in rows], MAX_SAMPLES)
    got = wave.cpu()
    for u in range(U):
        assert torch.equal(got[u], want[u]), u
        assert got[u, lens[u]:].abs().max().item() == 0.0 if lens[u] < MAX_SAMPLES else True     # the pad region is 0.0, not the 0xFF fill
    found = ar.check()
    assert not found, describe_guards(found)
    assert not ar.changed_inputs()


def test_device_clamps_and_refusals(lib, dev, pool, corpus):
    from quickvc_official_amd import lib as L
    from quickvc_official_amd.frontend import pcm_to_wave
    p, ref = corpus[("s16", 1)][LENGTHS.index(4099)]
    pcm, slot, table = _stage(pool, [p] * 5, dev)
    assert slot == 8208                                                        # 4104 s16 frames, 2052 stereo ones
    t = table.cpu()
    t[0, 2] = 1 << 30                                                          # more frames than the slot holds: cut to the slot
    t[1, 2] = -7                                                               # negative: 0
    t[2, 0] = 9                                                                # an unknown code
    t[3, 1] = 3                                                                # three channels are the host's
    t[4, 1], t[4, 2] = 2, 1 << 30                                              # the slot read as stereo: half as many frames
    wave, samples = pcm_to_wave(pcm, slot, t.to(dev), 5000)
    assert samples.tolist() == [4104, 0, 0, 0, 2052]
    got = wave.cpu()
    assert torch.equal(got[0, :4099], torch.from_numpy(ref)) and got[0, 4104:].abs().max().item() == 0.0
    for u in (1, 2, 3):
        assert got[u].abs().max().item() == 0.0, u
    pairs = torch.from_numpy(ref[:4098]).view(2049, 2)
    assert torch.equal(got[4, :2049], (pairs[:, 0] + pairs[:, 1]) * 0.5) and got[4, 2052:].abs().max().item() == 0.0
    # a slot size that is no multiple of 16 is refused before any launch: nothing is written
    wave.fill_(3.0)
    samples.fill_(-5)
    st = lib.qvc_pcm_to_wave_ragged(pcm.data_ptr(), slot - 8, table.data_ptr(), wave.data_ptr(), samples.data_ptr(), 5, 5000,
                                    torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert st == -1 and bool((wave == 3.0).all()) and samples.tolist() == [-5] * 5
    with pytest.raises(L.QvcError):
        pcm_to_wave(pcm, slot - 8, table, 5000)


# ------------------------------------------------------------------ embeddings from files
def _mini_model(seed):
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_state_dict
    model = q.SynthesizerTrn(641, 32, **q.MINI_MODEL_CONFIG)
    model.load_state_dict(make_synthetic_state_dict(model, seed))
    return model


def _speechlike(n, lead, tail, seed, sr=SR, f0=180.0):
    t = np.arange(n) / float(sr)
    w = 0.4 * np.sin(2 * np.pi * (f0 + 9 * seed) * t) + 0.05 * np.sin(2 * np.pi * (310.0 + seed) * t)
    w[:lead] = 0.0
    w[n - tail:] = 0.0
    return w


def _write(path, fmt, w, rate=SR):
    """One recording from float channels w (frames, channels) in a format."""
    w = np.asarray(w, dtype=np.float64).reshape(len(w), -1)
    data = {"u8": lambda: np.round(w * 127 + 128).astype(np.uint8), "s16": lambda: np.round(w * 32767).astype(np.int16),
            "s24": lambda: np.round(w * 8388607).astype(np.int32), "s32": lambda: np.round(w * 2147483647).astype(np.int32),
            "f32": lambda: w.astype(np.float32), "f64": lambda: w}[fmt]()
    with open(path, "wb") as f:
        f.write(wavgen.wav_bytes(fmt, data, rate=rate, extra="before" if fmt == "s24" else "none", extensible=fmt == "s24"))
    return path


def _targets(d):
    """Seven recordings: five formats on the native route, one that needs resampling and one f64 file on the host route."""
    mk = lambda i, sec, sr=SR: _speechlike(int(sec * sr) + 37 * i, int(0.1 * sr) + 64 * i, int(0.05 * sr) + i, i, sr)
    return [_write(str(d / "a_s16.wav"), "s16", mk(0, 0.9)),
            _write(str(d / "b_s16_stereo.wav"), "s16", np.stack([mk(1, 0.6), 0.5 * mk(1, 0.6)[::-1]], axis=1)),
            _write(str(d / "c_s24.wav"), "s24", mk(2, 1.2)),
            _write(str(d / "d_f32.wav"), "f32", mk(3, 0.5)),
            _write(str(d / "e_u8.wav"), "u8", mk(4, 0.8)),
            _write(str(d / "f_s16_22050.wav"), "s16", mk(5, 0.7, 22050), rate=22050),
            _write(str(d / "g_f64.wav"), "f64", mk(6, 1.0))]


def test_speaker_embed_files_equals_the_host_route(lib, dev, pool, tmp_path):
    from quickvc_official_amd.frontend import MelFrontend, load_wav
    net = _mini_model(31).cuda().eval()
    fe = MelFrontend(1280, 80, SR, 320, 1280, 0.0, None, device=dev)
    paths = _targets(tmp_path)
    staged = net.stage_target_files(paths, SR, pool)
    assert staged["order"] == [0, 1, 2, 3, 4, 5, 6] and staged["rows"] == 7      # the two host-route files are the last two here
    g = net.speaker_embed_files(paths, fe, pool)
    ref = net.speaker_embed_waves([load_wav(p, SR) for p in paths], fe, trim_top_db=20.0)
    assert g.shape == ref.shape == (7, 64) and torch.equal(g, ref)
    mixed = [paths[i] for i in (5, 0, 6, 2, 1)]                                   # host-route files first and in the middle: rows are permuted and put back
    assert torch.equal(net.speaker_embed_files(mixed, fe, pool, trim_top_db=None),
                       net.speaker_embed_waves([load_wav(p, SR) for p in mixed], fe, trim_top_db=None))
    short = _write(str(tmp_path / "short.wav"), "s16", _speechlike(300, 0, 1, 7))
    errs = []
    for call in (lambda ps: net.speaker_embed_files(ps, fe, pool), lambda ps: net.speaker_embed_waves([load_wav(p, SR) for p in ps], fe)):
        for ps in ([short], [paths[0], short, paths[2]]):
            with pytest.raises(ValueError) as ei:
                call(ps)
            errs.append(str(ei.value))
    assert errs[:2] == errs[2:] and "[1]" in errs[1]


# ------------------------------------------------------------------ fp32 -> int16
def _pcm16_inputs():
    specials = [1.0, -1.0, 1.0 - 2.0 ** -16, 2.0, -2.0, float("inf"), float("-inf"), float("nan"), 1e-40, -1e-40, 1.1754942e-38]
    halves = [(k + 0.5) / 32768.0 for k in range(-5, 6)]
    draws = np.random.RandomState(12).randn(4096) * 0.4
    return np.concatenate([np.asarray(specials + halves, dtype=np.float32), draws.astype(np.float32)])


def _pcm16_ref(x):
    with np.errstate(invalid="ignore"):
        q = np.clip(np.rint(x * np.float32(32768)), -32768, 32767)
        q = np.where(np.isnan(q), np.float32(0), q)                             # NaN -> 0, whatever the host's cast makes of it
        return q.astype(np.int16)


@pytest.mark.parametrize("n", [1, 7, 4097])
def test_wave_to_pcm16_equals_numpy(lib, dev, n):
    from quickvc_official_amd.frontend import wave_to_pcm16
    x = _pcm16_inputs()
    ref = _pcm16_ref(x)
    assert ref[:11].tolist() == [32767, -32768, 32767, 32767, -32768, 32767, -32768, 0, 0, 0, 0]
    assert ref[11:22].tolist() == [-4, -4, -2, -2, 0, 0, 2, 2, 4, 4, 6]      # halves go to even
    offsets = {1: range(22), 7: (0, 7, 14, 21), 4097: (0, 21)}[n]
    for off in offsets:
        ar = ArenaSet(dev, 0xFF, 0xFF)
        src = ar.input("wave", torch.from_numpy(x[off:off + n].copy()))
        out = ar.output("pcm", torch.int16, (n,))
        assert lib.qvc_wave_to_pcm16(src.data_ptr(), out.data_ptr(), n, torch.cuda.current_stream(dev).cuda_stream) == 0
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), ref[off:off + n]), (n, off)
        found = ar.check()
        assert not found, describe_guards(found)
        assert not ar.changed_inputs()
    # a source that is not 16-byte aligned (the element-wise form of the kernel) through the Python wrapper
    xd = torch.from_numpy(x).to(dev)
    got = wave_to_pcm16(xd[1:1 + n])
    assert got.dtype == torch.int16 and np.array_equal(got.cpu().numpy(), ref[1:1 + n])


# ------------------------------------------------------------------ CLI
@pytest.fixture(scope="module")
def cli_case(tmp_path_factory):
    """A 5-line list on the mini checkpoint: targets of mixed formats, one of them shared by two lines, one long source."""
    import quickvc_official_amd as q
    from quickvc_official_amd.checkpoint import save_checkpoint
    d = tmp_path_factory.mktemp("cli")
    cfg = {"train": {"segment_size": 10240}, "data": dict(q.DEFAULT_DATA_CONFIG), "model": dict(q.MINI_MODEL_CONFIG)}
    assert cfg["data"]["sampling_rate"] == SR
    (d / "config.json").write_text(json.dumps(cfg))
    save_checkpoint(_mini_model(33), None, 2e-4, 1, str(d / "G_1.pth"))
    tg = _targets(d)
    rng = np.random.RandomState(3)
    lines = []
    for i, (frames, t) in enumerate(zip((24, 31, 24, 60, 17), (tg[0], tg[2], tg[5], tg[1], tg[0]))):
        np.save(str(d / f"s{i}.npy"), rng.randn(frames, 256).astype(np.float32))
        lines.append(f"t_{i}|{d}/s{i}.npy|{t}\n")
    (d / "convert.txt").write_text("".join(lines))
    return d


def _run_cli(d, name, *flags):
    from quickvc_official_amd import convert as cli
    out = d / name
    cli.main(["--hpfile", str(d / "config.json"), "--ptfile", str(d / "G_1.pth"), "--txtpath", str(d / "convert.txt"), "--outdir", str(out),
              "--seed", "7", "--noise", "native", *flags])
    names = sorted(os.listdir(out))
    assert names == [f"t_{i}.wav" for i in range(5)]
    return {n: open(out / n, "rb").read() for n in names}


def test_cli_target_io_routes_write_identical_files(lib, dev, cli_case):
    auto = _run_cli(cli_case, "auto", "--target-io", "auto")
    scipy_route = _run_cli(cli_case, "scipy", "--target-io", "scipy")
    assert auto == scipy_route
    assert _run_cli(cli_case, "default") == auto                                # auto is the default


@pytest.mark.parametrize("max_frames", [0, 40])
def test_cli_pcm16_files_equal_the_quantised_float_files(lib, dev, cli_case, tmp_path, max_frames):
    """max_frames = 40 sends the 60-frame source down the window path (convert_long_items), the rest through the pipeline."""
    from scipy.io import wavfile
    from quickvc_official_amd.frontend import wave_to_pcm16
    extra = ["--max-frames", str(max_frames)] if max_frames else []
    _run_cli(cli_case, f"f32_{max_frames}", *extra)
    got = _run_cli(cli_case, f"pcm16_{max_frames}", "--pcm16", *extra)
    for name, blob in got.items():
        rate, x = wavfile.read(str(cli_case / f"f32_{max_frames}" / name))
        assert rate == SR and x.dtype == np.float32
        q = wave_to_pcm16(torch.from_numpy(x).to(dev)).cpu().numpy()
        ref = str(tmp_path / name)
        wavfile.write(ref, SR, q)
        assert open(ref, "rb").read() == blob, name
