"""GPU tests (-m gpu) of ragged target batches: silence trim, mel and speaker encoder for a padded batch of recordings
of different lengths, lengths on the device (qvc_trim_bounds, qvc_wave_to_mel_ragged, qvc_speaker_embed_ragged).

The contract is equality, not a tolerance: every row of a ragged call must be bit-identical (torch.equal) to the
uniform call on that row alone -- MFMA columns are independent, tiles start at each row's frame 0 and the mean runs
over a row's own partials in the same order -- whatever the padding and the workspace held before the call.  The two
tolerances that do appear are the project's existing ones against the CPU oracle (1e-3 relative L2 for an f16
embedding, 2e-5 for a log-mel)."""
import ctypes

import numpy as np
import pytest
import torch

import qvc_oracle as oracle
from helpers import load_case, regenerate, snr_db

pytestmark = pytest.mark.gpu

CYCLE = (1, 50, 127, 128, 129, 192, 193, 300, 321)


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


def _engine(entry, sd, dev, dtype):
    import quickvc_official_amd as q
    from quickvc_official_amd.engine import QvcEngine
    model = q.SynthesizerTrn(641, 32, **entry["config"])
    return QvcEngine(dict(model.model_config, operand_dtype=dtype), sd, dev)


def _front(dev):
    from quickvc_official_amd.frontend import MelFrontend
    return MelFrontend(1280, 80, 16000, 320, 1280, 0.0, None, device=dev)


def _padded_mels(frames, fmax, dev, seed0):
    """(U, 80, fmax) with row u's first frames[u] columns synthetic and the rest NaN, plus the rows on their own."""
    from quickvc_official_amd.synth import make_synthetic_mel
    rows = [make_synthetic_mel(max(f, 1), 80, seed=seed0 + 13 * u)[:, :, :f].to(dev) for u, f in enumerate(frames)]
    mel = torch.full((len(frames), 80, fmax), float("nan"), device=dev)
    for u, r in enumerate(rows):
        mel[u, :, :r.shape[2]] = r[0]
    return mel, rows


def _poisoned_ws(eng, U, fmax):
    n = int(eng.lib.qvc_spk_ragged_workspace_bytes(ctypes.byref(eng.cfg), U, fmax))
    assert n > 0
    from quickvc_official_amd.engine import aligned_empty
    ws = aligned_empty(n, eng.device)
    ws.fill_(0xFF)
    return ws


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_speaker_embed_ragged_rows_equal_single_calls(lib, dev, dtype):
    """mini model (gin 64), 19 rows (the second 16-column workgroup is partly filled), frame counts on both sides of the
    128-frame window and of the 64-frame hop, NaN in the mel padding, 0xFF bytes in the workspace."""
    entry, _ = load_case("mini")
    _m, sd, _u, _g, _n = regenerate(entry)
    eng = _engine(entry, sd, dev, dtype)
    frames = [CYCLE[u % len(CYCLE)] for u in range(19)]
    mel, rows = _padded_mels(frames, 321, dev, 100)
    fr = torch.tensor(frames, dtype=torch.int32, device=dev)
    g = eng.speaker_embed_ragged(mel, fr, ws=_poisoned_ws(eng, 19, 321))
    assert g.shape == (19, 64) and g.dtype == torch.float32 and bool(torch.isfinite(g).all())
    singles = [eng.speaker_embed(r) for r in rows]
    for u in range(19):
        assert torch.equal(g[u:u + 1], singles[u]), (u, frames[u])
    # a row given 0 frames is all zeros and the other rows do not notice
    fr0 = fr.clone()
    fr0[4] = 0
    g0 = eng.speaker_embed_ragged(mel, fr0, ws=_poisoned_ws(eng, 19, 321))
    assert bool((g0[4] == 0).all())
    keep = [u for u in range(19) if u != 4]
    assert torch.equal(g0[keep], g[keep])
    # lengths outside [0, max_frames] are clamped on the device
    fr_big = fr.clone()
    fr_big[8] = 10 ** 6
    fr_big[1] = -5
    gb = eng.speaker_embed_ragged(mel, fr_big, ws=_poisoned_ws(eng, 19, 321))
    assert torch.equal(gb[8:9], singles[8]) and bool((gb[1] == 0).all())      # row 8 has all 321 frames
    # the same batch with every row at 300 frames: the uniform call
    mel300, _rows = _padded_mels([300] * 19, 300, dev, 500)
    gu = eng.speaker_embed(mel300)
    gr = eng.speaker_embed_ragged(mel300, torch.full((19,), 300, dtype=torch.int32, device=dev), ws=_poisoned_ws(eng, 19, 300))
    assert torch.equal(gr, gu)


def test_speaker_embed_ragged_full_width(lib, dev):
    """Full width (gin 256: the 8-wave recurrence with resident k-steps), rows equal the single calls and sit within the
    existing 1e-3 relative L2 of the oracle's embed_utterance."""
    entry, _ = load_case("full_b1")
    _m, sd, _u, _g, _n = regenerate(entry)
    sdf = {k: v.float() for k, v in sd.items()}
    eng = _engine(entry, sd, dev, "f16")
    frames = [100, 129, 250, 321]
    mel, rows = _padded_mels(frames, 321, dev, 900)
    g = eng.speaker_embed_ragged(mel, torch.tensor(frames, dtype=torch.int32, device=dev), ws=_poisoned_ws(eng, 4, 321))
    for u, r in enumerate(rows):
        assert torch.equal(g[u:u + 1], eng.speaker_embed(r)), frames[u]
    ref = torch.cat([oracle.speaker_embed_utterance(sdf, r.cpu().transpose(1, 2)) for r in rows], 0).double().numpy()
    got = g.cpu().double().numpy()
    err = np.sqrt(((ref - got) ** 2).sum(-1) / (ref ** 2).sum(-1))
    print("relative L2 per row:", err)
    assert float(err.max()) <= 1e-3


def test_speaker_embed_ragged_bad_args(lib, dev):
    entry, _ = load_case("mini")
    _m, sd, _u, _g, _n = regenerate(entry)
    eng = _engine(entry, sd, dev, "f16")
    mel = torch.zeros(2, 80, 50, device=dev)
    fr = torch.tensor([50, 20], dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        eng.speaker_embed_ragged(torch.zeros(2, 79, 50, device=dev), fr)
    with pytest.raises(ValueError):
        eng.speaker_embed_ragged(mel, fr[:1])
    eng.speaker_embed_ragged(mel, fr)
    g = torch.empty(2, 64, device=dev)
    args = (ctypes.byref(eng.cfg), eng._spk_blob.data_ptr(), mel.data_ptr(), fr.data_ptr(), g.data_ptr(), 2, 50)
    assert eng.lib.qvc_speaker_embed_ragged(*args, eng._spk_ws.data_ptr(), 16, None) == -5      # QVC_ERR_SMALL_BUFFER
    assert eng.lib.qvc_speaker_embed_ragged(args[0], args[1], args[2], None, args[4], 2, 50,
                                            eng._spk_ws.data_ptr(), eng._spk_ws.numel(), None) == -1   # QVC_ERR_BAD_ARG
    fe = _front(dev)
    wave = torch.zeros(2, 4000, device=dev)
    n = torch.tensor([4000, 3000], dtype=torch.int32, device=dev)
    mel2, frames = fe.ragged(wave, n)
    a = (fe.table.data_ptr(), 1280, 320, 80, wave.data_ptr(), None, n.data_ptr(), mel2.data_ptr(), frames.data_ptr(), 2, 4000)
    assert eng.lib.qvc_wave_to_mel_ragged(*a, fe._ws.data_ptr(), 16, None) == -5
    assert eng.lib.qvc_wave_to_mel_ragged(*a[:6], None, *a[7:], fe._ws.data_ptr(), fe._ws.numel(), None) == -1
    st = torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(int(eng.lib.qvc_trim_workspace_bytes(2, 4000, 2048, 512)), dtype=torch.uint8, device=dev)
    t = (wave.data_ptr(), n.data_ptr(), st.data_ptr(), frames.data_ptr(), 2, 4000, 20.0, 2048, 512)
    assert eng.lib.qvc_trim_bounds(*t, ws.data_ptr(), 16, None) == -5
    assert eng.lib.qvc_trim_bounds(t[0], None, *t[2:], ws.data_ptr(), ws.numel(), None) == -1
    assert eng.lib.qvc_trim_bounds(*t[:7], 2048, 500, ws.data_ptr(), ws.numel(), None) == -2          # QVC_ERR_BAD_CONFIG
    torch.cuda.synchronize()


# ------------------------------------------------------------------ mel
MEL_LENS = (641, 2000, 48123, 80000)


@pytest.fixture(scope="module")
def mel_batch(dev):
    """One padded batch (rows of 641 / 2000 / 48123 / 80000 samples, NaN tails), shared and left unchanged."""
    gen = torch.Generator().manual_seed(77)
    N = max(MEL_LENS)
    t = torch.arange(N) / 16000.0
    wave = 0.3 * torch.sin(2 * np.pi * 220.0 * t)[None] * torch.rand(len(MEL_LENS), 1, generator=gen) + 0.05 * torch.randn(len(MEL_LENS), N, generator=gen)
    wave = wave.clamp(-1, 1)
    for u, n in enumerate(MEL_LENS):
        wave[u, n:] = float("nan")
    return wave.to(dev)


def test_wave_to_mel_ragged_rows_equal_single_calls(lib, dev, mel_batch):
    from quickvc_official_amd.frontend import mel_basis
    fe = _front(dev)
    wave = mel_batch
    mel, frames = fe.ragged(wave, torch.tensor(MEL_LENS, dtype=torch.int32, device=dev))
    assert mel.shape == (4, 80, fe.frames(80000)) and frames.dtype == torch.int32
    assert frames.tolist() == [fe.frames(n) for n in MEL_LENS]
    for u, n in enumerate(MEL_LENS):
        f = fe.frames(n)
        assert torch.equal(mel[u:u + 1, :, :f], fe(wave[u:u + 1, :n])), n
        assert bool((mel[u, :, f:] == 0).all()), n                       # frames past the row's end are exactly 0
    ref = oracle.wave_to_mel(wave[3:4].cpu(), torch.from_numpy(mel_basis(16000, 1280, 80, 0.0, None)), 1280, 320, 1280)
    assert float((mel[3:4].cpu() - ref).abs().max()) <= 2e-5
    # the same rows entered at a start offset, lengths shortened to fit
    starts = (0, 100, 517, 1024)
    lens = [n - s for n, s in zip(MEL_LENS, starts)]
    mel2, frames2 = fe.ragged(wave, torch.tensor(lens, dtype=torch.int32, device=dev), torch.tensor(starts, dtype=torch.int32, device=dev))
    assert frames2.tolist() == [fe.frames(n) for n in lens]
    for u, (s, n) in enumerate(zip(starts, lens)):
        f = fe.frames(n)
        assert torch.equal(mel2[u:u + 1, :, :f], fe(wave[u:u + 1, s:s + n])), (s, n)
        assert bool((mel2[u, :, f:] == 0).all())
    # a row no longer than the reflect pad has no frame; lengths past the row are clamped to it
    mel3, frames3 = fe.ragged(wave, torch.tensor([480, 0, -7, 10 ** 6], dtype=torch.int32, device=dev), torch.tensor([0, 0, 0, 80000 - 2000], dtype=torch.int32, device=dev))
    assert frames3.tolist() == [0, 0, 0, fe.frames(2000)]
    assert bool((mel3[:3] == 0).all())
    assert torch.equal(mel3[3:4, :, :fe.frames(2000)], fe(wave[3:4, 78000:80000]))


# ------------------------------------------------------------------ trim
def _trim_frames_db(w, frame_length=2048, hop=512):
    """frontend.trim's per-frame level relative to the loudest frame, in float64."""
    pad = frame_length // 2
    x = np.pad(w.astype(np.float64), (pad, pad))
    n = 1 + (len(x) - frame_length) // hop
    idx = np.arange(frame_length)[None, :] + hop * np.arange(n)[:, None]
    rms = np.sqrt(np.mean(x[idx] ** 2, axis=1))
    return 20.0 * np.log10(np.maximum(rms, 1e-10)) - 20.0 * np.log10(max(rms.max(), 1e-10))


def _trim_rows():
    rng = np.random.RandomState(3)
    sig = lambda n: (0.3 * np.sin(2 * np.pi * 200.0 * np.arange(n) / 16000.0) + 0.01 * rng.randn(n)).astype(np.float32)
    quiet = lambda n: (1e-4 * rng.randn(n)).astype(np.float32)
    return [
        sig(1500),                                                              # shorter than one frame: left whole
        np.zeros(10000, np.float32),                                            # digital silence
        sig(12345),                                                             # loud throughout
        np.concatenate([quiet(512 * 10), sig(512 * 30), quiet(512 * 10 + 100)]),   # quiet, signal, quiet: edges on hop boundaries
        np.concatenate([quiet(512 * 8), sig(512 * 22 + 77)]),                   # signal to the very end
    ]


def test_trim_bounds_match_frontend_trim(lib, dev):
    from quickvc_official_amd.frontend import trim, trim_bounds
    rows = _trim_rows()
    want = []
    for w in rows:
        if len(w) >= 2048:
            db = _trim_frames_db(w)
            # a condition on the INPUTS, not a tolerance on the kernel: no frame sits within 0.5 dB of the threshold,
            # so fp32 summation order cannot move a bound
            assert float(np.abs(db + 20.0).min()) > 0.5, float(np.abs(db + 20.0).min())
            keep = np.nonzero(db > -20.0)[0]
            start, end = int(keep[0]) * 512, min(len(w), (int(keep[-1]) + 1) * 512)
        else:
            start, end = 0, len(w)
        assert np.array_equal(trim(w, top_db=20), w[start:end])
        want.append((start, end - start))
    assert want[0] == (0, 1500) and want[1] == (0, 10000) and want[2] == (0, 12345)
    assert 0 < want[3][0] and want[3][0] + want[3][1] < len(rows[3])            # cut on both sides
    assert 0 < want[4][0] and want[4][0] + want[4][1] == len(rows[4])           # cut in front only
    N = max(len(w) for w in rows)
    wave = torch.full((len(rows), N), float("nan"))
    for u, w in enumerate(rows):
        wave[u, :len(w)] = torch.from_numpy(w)
    start, length = trim_bounds(wave.to(dev), torch.tensor([len(w) for w in rows], dtype=torch.int32, device=dev))
    assert start.dtype == length.dtype == torch.int32 and start.device.type == "cuda"
    assert list(zip(start.tolist(), length.tolist())) == want


# ------------------------------------------------------------------ whole call, graph, CLI
def _mini_model(seed):
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_state_dict
    model = q.SynthesizerTrn(641, 32, **q.MINI_MODEL_CONFIG)
    model.load_state_dict(make_synthetic_state_dict(model, seed))
    return model


def _speechlike(n, lead, tail, seed, f0=180.0):
    """`lead` samples of silence, a tone, `tail` samples of silence (sharp edges: the trim threshold is far away)."""
    t = np.arange(n) / 16000.0
    w = 0.4 * np.sin(2 * np.pi * (f0 + seed) * t)
    w[:lead] = 0.0
    w[n - tail:] = 0.0
    return w.astype(np.float32)


def test_speaker_embed_waves_equals_per_file_path(lib, dev):
    from quickvc_official_amd.frontend import trim
    net = _mini_model(21).cuda().eval()
    fe = _front(dev)
    waves = [_speechlike(int(s * 16000) + 37 * i, 1600 + 512 * i, 800 * i + 1, i) for i, s in enumerate((0.5, 1.3, 4.0, 2.2, 0.9))]
    g = net.speaker_embed_waves(waves, fe)
    assert g.shape == (5, 64)
    for u, w in enumerate(waves):
        tw = trim(w, top_db=20)
        assert len(tw) < len(w)
        ref = net.speaker_embed(fe(torch.from_numpy(tw)[None].to(dev)))
        assert torch.equal(g[u:u + 1], ref), u
    g2 = net.speaker_embed_waves([torch.from_numpy(w) for w in waves], fe, trim_top_db=None)
    for u, w in enumerate(waves):
        assert torch.equal(g2[u:u + 1], net.speaker_embed(fe(torch.from_numpy(w)[None].to(dev)))), u
    with pytest.raises(ValueError, match=r"\[1\]"):
        net.speaker_embed_waves([waves[0], waves[1][:300], waves[2]], fe)
    with pytest.raises(ValueError):
        net.speaker_embed_waves([waves[0][:100]], fe)


def test_trim_mel_lstm_in_one_graph_follow_the_device_lengths(lib, dev):
    """Captured once, replayed with other lengths: fails if anything reads a length on the host."""
    from quickvc_official_amd.frontend import trim_bounds
    net = _mini_model(22).cuda().eval()
    eng, fe = net.engine(), _front(dev)
    lens_a, lens_b = [30000, 21000, 9000, 16000], [8000, 30000, 15000, 700]
    wave = torch.stack([torch.from_numpy(_speechlike(30000, 2048 + 512 * i, 1024, i)) for i in range(4)]).to(dev)
    samples = torch.tensor(lens_a, dtype=torch.int32, device=dev)

    def run():
        start, length = trim_bounds(wave, samples)
        mel, frames = fe.ragged(wave, length, start)
        return eng.speaker_embed_ragged(mel, frames), frames

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run()                                                                  # warm-up: blobs and workspaces exist
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_static, f_static = run()
    graph.replay()
    g_a, f_a = g_static.clone(), f_static.clone()
    samples.copy_(torch.tensor(lens_b, dtype=torch.int32))
    graph.replay()
    g_b, f_b = g_static.clone(), f_static.clone()
    eager_b, ef_b = run()
    assert torch.equal(g_b, eager_b) and torch.equal(f_b, ef_b)
    samples.copy_(torch.tensor(lens_a, dtype=torch.int32))
    eager_a, ef_a = run()
    assert torch.equal(g_a, eager_a) and torch.equal(f_a, ef_a)
    assert not torch.equal(f_a, f_b) and not torch.equal(g_a, g_b)


def test_convert_cli_embeds_forty_targets_in_batches(lib, dev, tmp_path):
    """A `title|src|tgt` list as the reference writes them: a separate target on every line, 40 recordings of different
    lengths.  Every written file equals what the Python API computes for that line alone (per-file trim -> mel ->
    speaker encoder, the utterance converted alone with the same noise draw)."""
    import json
    from scipy.io import wavfile
    import quickvc_official_amd as q
    from quickvc_official_amd import convert as cli
    from quickvc_official_amd.checkpoint import save_checkpoint
    from quickvc_official_amd.frontend import load_wav, trim
    cfg = {"train": {"segment_size": 10240}, "data": dict(q.DEFAULT_DATA_CONFIG), "model": dict(q.MINI_MODEL_CONFIG)}
    hp = tmp_path / "config.json"
    hp.write_text(json.dumps(cfg))
    model = _mini_model(23)
    pt = tmp_path / "G_1.pth"
    save_checkpoint(model, None, 2e-4, 1, str(pt))
    sr = cfg["data"]["sampling_rate"]
    rng = np.random.RandomState(9)
    frames, lines = 24, []
    for i in range(40):
        n = int(sr * (0.5 + 0.05 * ((i * 17) % 40))) + 11 * i                  # 0.5 .. 2.5 s, no two alike, not sorted
        wavfile.write(str(tmp_path / f"tgt{i}.wav"), sr, (_speechlike(n, 1600 + 64 * i, 900, i) * 32767).astype(np.int16))
        np.save(str(tmp_path / f"s{i}.npy"), rng.randn(frames, 256).astype(np.float32))
        lines.append(f"t_{i}|{tmp_path}/s{i}.npy|{tmp_path}/tgt{i}.wav\n")
    (tmp_path / "convert.txt").write_text("".join(lines))
    out = tmp_path / "out"
    cli.main(["--hpfile", str(hp), "--ptfile", str(pt), "--txtpath", str(tmp_path / "convert.txt"), "--outdir", str(out),
              "--seed", "7", "--batch", "40"])
    net = model.cuda().eval()
    fe = _front(dev)
    # equal source lengths: one ragged launch of 40 in list order, one noise draw keyed by (seed, first line)
    noise = cli.batch_noise(7, 0, 40, q.MINI_MODEL_CONFIG["inter_channels"], frames, dev)
    for i in range(40):
        rate, got = wavfile.read(str(out / f"t_{i}.wav"))
        assert rate == sr and got.dtype == np.float32 and got.shape == (320 * frames,)
        wav = torch.from_numpy(trim(load_wav(str(tmp_path / f"tgt{i}.wav"), sr), top_db=20))[None].to(dev)
        g = net.speaker_embed(fe(wav))
        unit = torch.from_numpy(np.load(str(tmp_path / f"s{i}.npy"))).t()[None].cuda()
        ref = net.infer_batch(unit, g, noise[i][None])
        assert snr_db(ref[0, 0].cpu().numpy(), got) >= 100.0, i
