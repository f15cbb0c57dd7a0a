"""GPU tests (run with -m gpu on an MI355X) of the fan-out path: R output rows from U <= R encoded sources
(qvc_infer_fanout_ragged, include/qvc.h) -- enc_p once per source as far as the projection's statistics, one
row-sampling launch, flow and decoder per row.

Bars (floating point, stated as the task requires):
  * against qvc_infer_batch_ragged on the expanded batch (units duplicated): torch.equal.  The statistics cross memory
    in fp32 (nothing is rounded), the draw is one shared inlined helper, and flow / decoder see identical shapes;
    enc_p's tile choices differ between U and R rows but no tile changes a K order;
  * against the fp32 oracle per row: f16 >= 45 dB, bf16x >= 40 dB (the bars of tests/test_gpu_parity.py);
  * through the CLI against the utterance converted alone: >= 100 dB (the bar of test_convert_cli_corpus_pipeline).
"""
import ctypes

import numpy as np
import pytest
import torch

import qvc_oracle as oracle
from helpers import snr_db

pytestmark = pytest.mark.gpu

LENS = [37, 20, 33]                      # 37 = the padded length: not a multiple of a 32-frame tile
MAP = [0, 2, 0, 1, 2, 0, 0]              # repeated, non-monotone, source 1 used once


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


DEBUG_DEFAULTS = {"post_tail": 1, "post_tail_nf": 4, "pair_wide_launch": 1, "pair_cm4": 1, "conv_cl": 1, "wn_chunk": 0,
                  "pair_chain3": 0, "wn_kernel": 0, "launch_stop": -1}


@pytest.fixture(autouse=True)
def _debug_switches_at_defaults():
    from quickvc_official_amd import lib as L
    for k, v in DEBUG_DEFAULTS.items():
        L.debug_set(k, v)
    yield
    for k, v in DEBUG_DEFAULTS.items():
        L.debug_set(k, v)


def _case(cfg_name, weights_seed):
    """Model, weights and the inputs of the 3-source / 7-row case for one model config (host tensors)."""
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_inputs, make_synthetic_state_dict
    cfg = dict(getattr(q, cfg_name))
    model = q.SynthesizerTrn(641, 32, **cfg)
    sd = make_synthetic_state_dict(model, weights_seed)
    unit, _g, _n = make_synthetic_inputs(len(LENS), max(LENS), 256, cfg["inter_channels"], cfg["gin_channels"], seed0=900)
    _u, g, noise = make_synthetic_inputs(len(MAP), max(LENS), 256, cfg["inter_channels"], cfg["gin_channels"], seed0=950)
    return dict(cfg=cfg, model_config=model.model_config, sd=sd, unit=unit, g=g, noise=noise)


@pytest.fixture(scope="module")
def mini():
    return _case("MINI_MODEL_CONFIG", 1234)


@pytest.fixture(scope="module")
def mini_oracle(mini):
    """The fp32 oracle's waveform of every row of the 7-row case, each converted alone (computed once, never modified)."""
    refs = []
    for r, s in enumerate(MAP):
        n = LENS[s]
        refs.append(oracle.infer_from_g(mini["sd"], mini["cfg"], mini["unit"][s:s + 1, :, :n], mini["g"][r:r + 1].unsqueeze(-1),
                                        mini["noise"][r:r + 1, :, :n]))
    return refs


def _engine(case, dev, dtype="f16"):
    from quickvc_official_amd.engine import QvcEngine
    return QvcEngine(dict(case["model_config"], operand_dtype=dtype), case["sd"], dev)


def _both(eng, case, dev, src_map=MAP, lens=LENS, unit_fm=False):
    """(fan-out call, qvc_infer_batch_ragged on the expanded batch) for a case's inputs."""
    unit, g, noise = case["unit"].to(dev), case["g"][:len(src_map)].to(dev), case["noise"][:len(src_map)].to(dev)
    frames, src = torch.tensor(lens, dtype=torch.int32), torch.tensor(src_map, dtype=torch.int32)
    u_in = unit.transpose(1, 2).contiguous() if unit_fm else unit
    fan = eng.infer_fanout_ragged(u_in, frames, src, g, noise, unit_fm=unit_fm)
    expanded = eng.infer_batch_ragged(unit[src.long()].contiguous(), g, noise, frames[src.long()])
    torch.cuda.synchronize()
    return fan, expanded


def _check_rows(fan, expanded, src_map, lens, spf=320):
    assert fan.shape == expanded.shape == (len(src_map), 1, spf * max(lens)) and bool(torch.isfinite(fan).all())
    for r, s in enumerate(src_map):
        n = spf * lens[s]
        assert float(fan[r, :, :n].abs().max()) > 0, r
        assert torch.equal(fan[r], expanded[r]), (r, s, snr_db(expanded[r].cpu(), fan[r].cpu()))
        if lens[s] < max(lens):
            assert float(fan[r, :, n:].abs().max()) == 0.0, r       # row tails past spf * len are exactly zero


def test_fanout_equals_the_expanded_batch(lib, dev, mini):
    eng = _engine(mini, dev)
    fan, expanded = _both(eng, mini, dev)
    _check_rows(fan, expanded, MAP, LENS)
    # rows 0, 2, 5, 6 share source 0 but neither g nor noise: they must differ
    assert not torch.equal(fan[0], fan[2]) and not torch.equal(fan[5], fan[6])
    # the step count: cond GEMV + enc_p (pre, 4 stack launches, proj) + row sampling + the rest = the plain path's
    # (whose projection samples in its epilogue) + 1
    from quickvc_official_amd import lib as L
    eng.infer_fanout_ragged(mini["unit"].to(dev), torch.tensor(LENS, dtype=torch.int32), torch.tensor(MAP, dtype=torch.int32),
                            mini["g"].to(dev), mini["noise"].to(dev))
    steps_fan = L.debug_get("launch_steps")
    eng.infer_batch_ragged(mini["unit"].to(dev)[MAP].contiguous(), mini["g"].to(dev), mini["noise"].to(dev),
                           torch.tensor([LENS[s] for s in MAP], dtype=torch.int32))
    info = (ctypes.c_int32 * 8)()
    assert lib.qvc_plan_info(ctypes.byref(eng.cfg), info) == 0
    assert steps_fan == L.debug_get("launch_steps") + (1 if info[0] else 0), (steps_fan, list(info))
    torch.cuda.synchronize()


def test_fanout_frame_major_units(lib, dev, mini):
    eng = _engine(mini, dev)
    fan_cm, _ = _both(eng, mini, dev)
    fan_fm, _ = _both(eng, mini, dev, unit_fm=True)
    assert torch.equal(fan_cm, fan_fm)


def test_fanout_odd_channel_counts(lib, dev):
    """inter 48 / hidden 40: C is not a multiple of the 32-channel noise tile of sample_rows_kernel.  The projection
    route is the one the plan takes (qvc_plan_info info[0]; there is no switch that forces the other)."""
    case = _case("ODD_MODEL_CONFIG", 4321)
    eng = _engine(case, dev)
    info = (ctypes.c_int32 * 8)()
    assert lib.qvc_plan_info(ctypes.byref(eng.cfg), info) == 0
    assert case["cfg"]["inter_channels"] % 32 != 0
    fan, expanded = _both(eng, case, dev)
    _check_rows(fan, expanded, MAP, LENS)
    fan_fm, _ = _both(eng, case, dev, unit_fm=True)
    assert torch.equal(fan, fan_fm), list(info)


def test_fanout_natural_projection_rows(lib, dev):
    """The other projection route: at inter 256 the paired-row kernels are not built (8 fragments per wave), the plan
    keeps natural rows (info[0] == 0) and the statistics come from the plain conv epilogue."""
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_inputs, make_synthetic_state_dict
    cfg = dict(q.MINI_MODEL_CONFIG, inter_channels=256)
    model = q.SynthesizerTrn(641, 32, **cfg)
    case = dict(cfg=cfg, model_config=model.model_config, sd=make_synthetic_state_dict(model, 77))
    case["unit"], _g, _n = make_synthetic_inputs(len(LENS), max(LENS), 256, 256, cfg["gin_channels"], seed0=900)
    _u, case["g"], case["noise"] = make_synthetic_inputs(len(MAP), max(LENS), 256, 256, cfg["gin_channels"], seed0=950)
    eng = _engine(case, dev)
    info = (ctypes.c_int32 * 8)()
    assert lib.qvc_plan_info(ctypes.byref(eng.cfg), info) == 0 and info[0] == 0, list(info)
    fan, expanded = _both(eng, case, dev)
    _check_rows(fan, expanded, MAP, LENS)


def test_fanout_clamps_the_map_and_never_reads_padding(lib, dev, mini):
    """U = 3, map [2, 2, 0, 7, -1] on the DEVICE (a host map is range-checked instead): 7 clamps to 2, -1 to 0; source 1
    is used by no row.  NaN in the padding of unit and noise and in the whole unit row of the unused source changes
    nothing."""
    eng = _engine(mini, dev)
    raw, clamped = [2, 2, 0, 7, -1], [2, 2, 0, 2, 0]
    unit, g, noise = mini["unit"].to(dev), mini["g"][:5].to(dev), mini["noise"][:5].to(dev)
    frames = torch.tensor(LENS, dtype=torch.int32)
    with pytest.raises(ValueError):
        eng.infer_fanout_ragged(unit, frames, torch.tensor(raw, dtype=torch.int32), g, noise)
    with pytest.raises(ValueError):
        eng.infer_fanout_ragged(unit, torch.tensor([37, 1, 33], dtype=torch.int32), torch.tensor(clamped, dtype=torch.int32), g, noise)
    want = eng.infer_fanout_ragged(unit, frames, torch.tensor(clamped, dtype=torch.int32), g, noise).clone()
    junk_u, junk_n = unit.clone(), noise.clone()
    for s, n in enumerate(LENS):
        junk_u[s, :, n:] = float("nan")
    junk_u[1] = float("nan")                                           # the unused source: encoded, never looked at
    for r, s in enumerate(clamped):
        junk_n[r, :, LENS[s]:] = float("nan")
    got = eng.infer_fanout_ragged(junk_u, frames.to(dev), torch.tensor(raw, dtype=torch.int32, device=dev), g, junk_n)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    for r, s in enumerate(clamped):
        if LENS[s] < max(LENS):
            assert float(got[r, :, 320 * LENS[s]:].abs().max()) == 0.0


@pytest.mark.parametrize("dtype,min_db", [("f16", 45.0), ("bf16x", 40.0)])
def test_fanout_rows_against_the_oracle(lib, dev, mini, mini_oracle, dtype, min_db):
    eng = _engine(mini, dev, dtype)
    fan = eng.infer_fanout_ragged(mini["unit"].to(dev), torch.tensor(LENS, dtype=torch.int32), torch.tensor(MAP, dtype=torch.int32),
                                  mini["g"].to(dev), mini["noise"].to(dev))
    torch.cuda.synchronize()
    for r, s in enumerate(MAP):
        db = snr_db(mini_oracle[r], fan[r:r + 1, :, :320 * LENS[s]].cpu())
        assert db >= min_db, (r, s, db)


def test_fanout_graph_replays_with_other_maps_and_lengths(lib, dev, mini):
    """The call reads neither the map nor the lengths on the host: captured once, it is replayed after both device arrays
    were overwritten and gives what the eager call gives for the new values."""
    eng = _engine(mini, dev)
    R, U, T = len(MAP), len(LENS), max(LENS)
    unit, g, noise = mini["unit"].to(dev), mini["g"].to(dev), mini["noise"].to(dev)
    frames = torch.tensor(LENS, dtype=torch.int32, device=dev)
    src = torch.tensor(MAP, dtype=torch.int32, device=dev)
    out = torch.empty(R, 1, 320 * T, device=dev)
    ws = eng.alloc_workspace(R, T, sources=U)                          # the graph owns the buffers it captured
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        first = eng.infer_fanout_ragged(unit, frames, src, g, noise, ws=ws).clone()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            eng.infer_fanout_ragged(unit, frames, src, g, noise, out=out, ws=ws)
        out.zero_()
        graph.replay()
        side.synchronize()
        assert torch.equal(out, first)
        map_b, lens_b = [1, 1, 2, 0, 1, 2, 2], [21, 37, 30]
        src.copy_(torch.tensor(map_b, dtype=torch.int32))
        frames.copy_(torch.tensor(lens_b, dtype=torch.int32))
        graph.replay()
        side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
    eager = eng.infer_fanout_ragged(unit, frames, src, g, noise)
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and not torch.equal(out, first)
    for r, s in enumerate(map_b):
        if lens_b[s] < T:
            assert float(out[r, :, 320 * lens_b[s]:].abs().max()) == 0.0


def test_fanout_model_surface(lib, dev, mini):
    """SynthesizerTrn.infer_fanout mirrors infer_ragged: lists in, a list of R waveforms out."""
    import quickvc_official_amd as q
    model = q.SynthesizerTrn(641, 32, **mini["cfg"])
    model.load_state_dict(mini["sd"])
    model = model.cuda().eval()
    units = [mini["unit"][s, :, :n] for s, n in enumerate(LENS)]
    noises = [mini["noise"][r, :, :LENS[s]] for r, s in enumerate(MAP)]
    waves = model.infer_fanout(units, MAP, mini["g"].cuda(), noises)
    want = model.infer_ragged([units[s] for s in MAP], mini["g"].cuda(), noises)
    torch.cuda.synchronize()
    assert [tuple(w.shape) for w in waves] == [(1, 320 * LENS[s]) for s in MAP]
    for r in range(len(MAP)):
        assert torch.equal(waves[r], want[r]), r
    with pytest.raises(ValueError):
        model.infer_fanout(units, [0, 3, 1], mini["g"][:3].cuda())


def test_convert_cli_fans_out_repeated_sources(lib, dev, tmp_path):
    """12 unit files, 4 targets, 40 list lines in which every source appears 2-5 times (the any-to-many shape), through
    the CLI: every line gets its wav, the pipeline reports the source encodes it saved, three lines (first / middle / last
    of the plan) equal the utterance converted alone with the noise batch_noise regenerates, and --fanout off writes
    the same files."""
    import json
    from scipy.io import wavfile
    import quickvc_official_amd as q
    from quickvc_official_amd import convert as cli
    from quickvc_official_amd.checkpoint import save_checkpoint
    from quickvc_official_amd.frontend import MelFrontend, load_wav, trim
    from quickvc_official_amd.synth import make_synthetic_state_dict
    cfg = {"train": {"segment_size": 10240}, "data": dict(q.DEFAULT_DATA_CONFIG), "model": dict(q.MINI_MODEL_CONFIG)}
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    model = q.SynthesizerTrn(641, 32, **q.MINI_MODEL_CONFIG)
    model.load_state_dict(make_synthetic_state_dict(model, 21))
    save_checkpoint(model, None, 2e-4, 1, str(tmp_path / "G_1.pth"))
    sr = cfg["data"]["sampling_rate"]
    t = np.arange(int(1.5 * sr)) / sr
    for k in range(4):
        wavfile.write(str(tmp_path / f"spk{k}.wav"), sr, (0.4 * np.sin(2 * np.pi * (140.0 + 45.0 * k) * t) * 32767).astype(np.int16))
    rng = np.random.RandomState(31)
    src_len = [int(v) for v in rng.choice(np.arange(20, 121), size=12, replace=False)]
    for i, n in enumerate(src_len):
        np.save(str(tmp_path / f"u{i:02d}.npy"), rng.randn(n, 256).astype(np.float32))
    counts = [2, 3, 4, 5, 2, 3, 4, 5, 2, 3, 4, 3]
    lines = [s for s, c in enumerate(counts) for _ in range(c)]
    assert len(lines) == 40
    rng.shuffle(lines)
    seen = {}
    items = []
    for k, s in enumerate(lines):                                      # copy j of a source goes to target j % 4
        j = seen[s] = seen.get(s, -1) + 1
        items.append((f"o{k:02d}", str(tmp_path / f"u{s:02d}.npy"), str(tmp_path / f"spk{j % 4}.wav")))
    (tmp_path / "convert.txt").write_text("".join(f"{a}|{b}|{c}\n" for a, b, c in items))
    base = ["--hpfile", str(tmp_path / "config.json"), "--ptfile", str(tmp_path / "G_1.pth"), "--txtpath", str(tmp_path / "convert.txt"),
            "--seed", "5", "--batch", "8", "--io-threads", "4"]
    stats = cli.main(base + ["--outdir", str(tmp_path / "out")])
    assert stats["utterances"] == 40 and stats["encodes_saved"] > 0, stats
    stats_off = cli.main(base + ["--outdir", str(tmp_path / "off"), "--fanout", "off"])
    assert stats_off["utterances"] == 40 and stats_off["encodes_saved"] == 0, stats_off
    waves = {}
    for k, s in enumerate(lines):
        rate, w = wavfile.read(str(tmp_path / "out" / f"o{k:02d}.wav"))
        assert rate == sr and w.dtype == np.float32 and w.shape == (320 * src_len[s],), k
        assert np.isfinite(w).all() and np.abs(w).max() > 0, k
        _r, w_off = wavfile.read(str(tmp_path / "off" / f"o{k:02d}.wav"))
        assert np.array_equal(w, w_off), (k, snr_db(w_off, w))
        waves[k] = w
    net = q.SynthesizerTrn(641, 32, **q.MINI_MODEL_CONFIG).cuda().eval()
    q.load_checkpoint(str(tmp_path / "G_1.pth"), net, None)
    d = cfg["data"]
    front = MelFrontend(d["filter_length"], d["n_mel_channels"], sr, d["hop_length"], d["win_length"], d["mel_fmin"], d["mel_fmax"])
    lengths, mine, batches = cli.rank_plan(items, 0, 1, 8)
    assert lengths == [src_len[s] for s in lines] and sum(len(b) for b in batches) == 40
    assert stats["encodes_saved"] == sum(len(b) - len(cli.fanout_rows([items[i][1] for i in b])[0]) for b in batches)
    inter = q.MINI_MODEL_CONFIG["inter_channels"]
    for bi, row in ((0, 0), (len(batches) // 2, 1), (len(batches) - 1, -1)):
        idxs = batches[bi]
        row %= len(idxs)
        i = idxs[row]
        tmax = max(lengths[j] for j in idxs)
        noise = cli.batch_noise(5, idxs[0], len(idxs), inter, tmax, dev)[row, :, :lengths[i]].unsqueeze(0)
        wav = torch.from_numpy(trim(load_wav(items[i][2], sr), top_db=20)).unsqueeze(0).cuda()
        g = net.speaker_embed(front(wav))
        unit = torch.from_numpy(np.load(items[i][1])).t().unsqueeze(0).cuda()
        alone = net.infer_batch(unit, g, noise)
        torch.cuda.synchronize()
        assert snr_db(alone[0, 0].cpu().numpy(), waves[i]) >= 100.0, (bi, i)
