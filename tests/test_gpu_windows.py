"""Exact windows over packed utterances on an MI355X (run with -m gpu): qvc_infer_windows_fm / _rng_fm through QvcEngine,
windows.WindowConverter, SynthesizerTrn.infer_long and convert.py --max-frames.  GPU output is compared with GPU output
of the whole-utterance path (qvc_infer_batch_ragged[_rng] of the utterance alone, same g, same noise or (seed, key)) at
>= 90 dB, the project's bar for streamed against offline (tests/test_gpu_live.py); every measured figure is printed.
out_packed starts as a sentinel everywhere: what no row delivers must still hold it.
"""
import functools
import json

import numpy as np
import pytest
import torch

import memguard as M
from helpers import snr_db
from live_common import NAN, SEED, _debug_switches_at_defaults, _keys, dev, lib, _row_model  # noqa: F401
from windows_common import SENTINEL, groups_of, mini_problem, packed_inputs, table_rows

pytestmark = pytest.mark.gpu


class _Mini:
    """The mini base model on the GPU (what the converters need of a model)."""

    def __init__(self, dtype="f16"):
        from quickvc_official_amd.engine import QvcEngine
        mc, sd = mini_problem()
        self.model_config = dict(mc, operand_dtype=dtype)
        self._engine = QvcEngine(self.model_config, sd, torch.device("cuda:0"))
        self.samples_per_frame = self._engine.samples_per_frame

    def engine(self):
        return self._engine


@functools.lru_cache(maxsize=None)
def _mini():
    return _Mini()


def _launch(eng, units, table, g_rows, n, rows, noise=None, keys=None, out=None, ws=None):
    """The table in groups of `rows` rows, direct launches on a workspace of NaN bytes -> out_packed (a sentinel where
    nothing was delivered).  g_rows / keys: one per table row."""
    from quickvc_official_amd.engine import aligned_empty
    device = eng.device
    total, spf = units.shape[0], eng.samples_per_frame
    if ws is None:
        ws = aligned_empty(eng.windows_sizes(rows, n)[0], device)
        ws.fill_(0xFF)
    if out is None:
        out = torch.full((total * spf,), SENTINEL, device=device)
    groups = groups_of(table, rows).to(device)
    G = groups.shape[0]
    gg = torch.zeros(G * rows, g_rows.shape[1], device=device)
    gg[:g_rows.shape[0]] = g_rows.to(device)
    kk = torch.zeros(G * rows, dtype=torch.int64, device=device)
    if keys is not None:
        kk[:len(keys)] = torch.tensor([k - (1 << 64) if k >> 63 else k for k in keys], dtype=torch.int64)
    for i in range(G):
        sl = slice(i * rows, (i + 1) * rows)
        eng.infer_windows(ws, units, noise, groups[i].contiguous(), gg[sl].contiguous(), out, n,
                          rng=None if keys is None else (SEED, kk[sl].contiguous(), 1.0))
    torch.cuda.synchronize()
    return out


def _alone(eng, units, base, length, g_row, noise=None, key=None):
    """qvc_infer_batch_ragged[_rng] of one utterance of the packed buffer alone -> (length * spf,)"""
    u = units[base:base + length].unsqueeze(0).contiguous()
    frames = torch.tensor([length], dtype=torch.int32)
    if noise is None:
        out = eng.infer_batch_ragged(u, g_row.reshape(1, -1), None, frames, unit_fm=True, rng=(SEED, [key], 1.0))
    else:
        out = eng.infer_batch_ragged(u, g_row.reshape(1, -1), noise[:, base:base + length].unsqueeze(0).contiguous(), frames, unit_fm=True)
    return out[0, 0].clone()


def _check(got, want, what, bar=90.0):
    got, want = got.cpu(), want.cpu()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0, what
    db = snr_db(want, got)
    print(f"{what}: {db:.1f} dB")
    assert db >= bar, (what, db)


def _bases(lengths):
    return [sum(lengths[:u]) for u in range(len(lengths))]


def _owners(lengths, n):
    return [u for u, length in enumerate(lengths) for _ in range(-(-length // n))]


# ---------------------------------------------------------------- the two forms on the mini base model
def test_generator_form_equals_the_utterance_alone(lib, dev):
    """Lengths 2, 16, 17, 89, 105 and 300 at n = 16 in groups of 4 rows, f16; an idle row with junk in its other fields
    among them; EXTRA frames behind the last utterance that no row names keep the sentinel."""
    lengths, n, rows, extra = (2, 16, 17, 89, 105, 300), 16, 4, 5
    eng = _mini().engine()
    mc = _mini().model_config
    units, _noise, g = (t.to(dev) for t in packed_inputs(lengths, mc["inter_channels"], mc["gin_channels"], 9200, extra=extra))
    table, owner = table_rows(lengths, n), _owners(lengths, n)
    table.insert(5, (7, 1 << 30, -3, 0))
    owner.insert(5, 0)
    keys = _keys(len(lengths))
    out = _launch(eng, units, table, g[owner], n, rows, keys=[keys[u] for u in owner])
    spf = eng.samples_per_frame
    for u, (base, length) in enumerate(zip(_bases(lengths), lengths)):
        _check(out[base * spf:(base + length) * spf], _alone(eng, units, base, length, g[u], key=keys[u]), f"rng utterance {u} ({length} frames)")
    assert bool((out[sum(lengths) * spf:] == SENTINEL).all()) and not bool((out[:sum(lengths) * spf] == SENTINEL).any())


def test_pointer_form_equals_the_utterance_alone(lib, dev):
    lengths, n, rows = (17, 105), 16, 4
    eng = _mini().engine()
    mc = _mini().model_config
    units, noise, g = (t.to(dev) for t in packed_inputs(lengths, mc["inter_channels"], mc["gin_channels"], 9300))
    owner = _owners(lengths, n)
    out = _launch(eng, units, table_rows(lengths, n), g[owner], n, rows, noise=noise)
    spf = eng.samples_per_frame
    for u, (base, length) in enumerate(zip(_bases(lengths), lengths)):
        _check(out[base * spf:(base + length) * spf], _alone(eng, units, base, length, g[u], noise=noise), f"ptr utterance {u} ({length} frames)")


# ---------------------------------------------------------------- every decoder
@pytest.mark.parametrize("trim", [True, False], ids=["trimmed", "plain"])
@pytest.mark.parametrize("row", ["one_up8", "mb_up16_up1", "istft_ups3", "rb_k1_k15_k13", "wn_enc1_flow1"])
def test_every_decoder(lib, dev, row, trim):
    """Rows of the configuration space at n = 8, utterances of 9 and 2C + 11 frames (shorter than one window; longer than
    one with both contexts inside it), generator form, trimmed and plain."""
    from quickvc_official_amd import lib as L
    from quickvc_official_amd.synth import make_synthetic_inputs
    model, C = _row_model(row)
    eng, mc = model.engine(), model.model_config
    assert eng.windows_sizes(2, 8)[1] == C
    lengths, n, rows = (9, 2 * C + 11), 8, 4
    unit, g, _noise = make_synthetic_inputs(2, max(lengths), 256, mc["inter_channels"], mc["gin_channels"], seed0=9400)
    units = torch.cat([unit[u, :, :length].t() for u, length in enumerate(lengths)]).contiguous().to(dev)
    g = g.to(dev)
    owner, keys = _owners(lengths, n), _keys(2)
    L.debug_set("live_trim", 1 if trim else 0)
    out = _launch(eng, units, table_rows(lengths, n), g[owner], n, rows, keys=[keys[u] for u in owner])
    L.debug_set("live_trim", 1)
    spf = eng.samples_per_frame
    for u, (base, length) in enumerate(zip(_bases(lengths), lengths)):
        _check(out[base * spf:(base + length) * spf], _alone(eng, units, base, length, g[u], key=keys[u]), f"{row} utterance {u} ({length} frames)")


# ---------------------------------------------------------------- a target speaker per region
def test_region_targets(lib, dev):
    """One utterance of 64 frames at n = 16, the rows alternating two g rows: each window equals, on its delivered
    frames, the whole-utterance conversion under its own g."""
    length, n = 64, 16
    eng = _mini().engine()
    mc = _mini().model_config
    units, _noise, g = (t.to(dev) for t in packed_inputs((length, 2), mc["inter_channels"], mc["gin_channels"], 9500))
    units = units[:length].contiguous()
    table = table_rows((length,), n)
    which = [i % 2 for i in range(len(table))]
    key = _keys(1)[0]
    out = _launch(eng, units, table, g[which], n, 4, keys=[key] * len(table))
    whole = [_alone(eng, units, 0, length, g[k], key=key) for k in range(2)]
    spf = eng.samples_per_frame
    for (_b, _l, start, count), k in zip(table, which):
        sl = slice(start * spf, (start + count) * spf)
        _check(out[sl], whole[k][sl], f"region at {start} under g[{k}]")
    assert snr_db(whole[0], whole[1]) < 60.0                               # the two targets do differ


# ---------------------------------------------------------------- one captured call, replayed with other contents
def test_graph_replays_with_another_table_lengths_and_contents(lib, dev):
    from quickvc_official_amd.engine import aligned_empty
    eng = _mini().engine()
    mc = _mini().model_config
    n, rows, total = 16, 4, 120
    spf = eng.samples_per_frame
    ws = aligned_empty(eng.windows_sizes(rows, n)[0], dev)
    units, out = torch.zeros(total, 256, device=dev), torch.full((total * spf,), SENTINEL, device=dev)
    table, g = torch.zeros(rows, 4, dtype=torch.int32, device=dev), torch.zeros(rows, mc["gin_channels"], device=dev)
    keys = torch.zeros(rows, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        eng.infer_windows(ws, units, None, table, g, out, n, rng=(SEED, keys, 1.0))      # warm-up on idle rows
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            eng.infer_windows(ws, units, None, table, g, out, n, rng=(SEED, keys, 1.0))
    assert bool((out == SENTINEL).all())                                   # idle rows deliver nothing
    for seed0, lengths in ((9600, (50, 33, 21)), (9700, (7, 100))):
        u, _nz, gg = (t.to(dev) for t in packed_inputs(lengths, mc["inter_channels"], mc["gin_channels"], seed0))
        tab, owner = table_rows(lengths, n), _owners(lengths, n)
        kk = [_keys(3)[o] for o in owner]
        direct = _launch(eng, u, tab, gg[owner], n, rows, keys=kk)
        units.zero_()
        units[:u.shape[0]] = u
        out.fill_(SENTINEL)
        groups = groups_of(tab, rows).to(dev)
        for i in range(groups.shape[0]):
            sl = slice(i * rows, (i + 1) * rows)
            table.copy_(groups[i])
            g.zero_()
            g[:len(owner[sl])] = gg[owner[sl]]
            keys.zero_()
            keys[:len(kk[sl])] = torch.tensor([k - (1 << 64) if k >> 63 else k for k in kk[sl]], dtype=torch.int64)
            torch.cuda.synchronize()
            graph.replay()
        torch.cuda.synchronize()
        named = sum(lengths) * spf
        assert M.bits_equal(out[:named], direct[:named]), lengths
        assert bool((out[named:] == SENTINEL).all())


# ---------------------------------------------------------------- the memory contract
def test_memory_contract(lib, dev):
    """Every caller-owned buffer in a guarded arena under the 0x00 / 0x3C / 0xFF fills (the workspace and out_packed start
    as the fill: a stale workspace), NaN in the packed frames no row names, a table with junk rows among the real ones:
    no guard byte changes, no input changes, and the delivered samples are the same bits under every fill."""
    eng = _mini().engine()
    mc = _mini().model_config
    lengths, n, rows, extra = (21, 40), 16, 4, 6
    spf = eng.samples_per_frame
    units, noise, g = packed_inputs(lengths, mc["inter_channels"], mc["gin_channels"], 9800, extra=extra)
    units, noise = units.clone(), noise.clone()
    units[sum(lengths):] = NAN
    noise[:, sum(lengths):] = NAN
    big, small = (1 << 31) - 1, -(1 << 31)
    tab = table_rows(lengths, n) + [(small, lengths[0], small, big), (big, big, big, big), (-1, -1, -1, 5), (3, small, 0, 5)]
    owner = _owners(lengths, n) + [0, 1, 0, 1]
    groups = groups_of(tab, rows)
    n_ws = eng.windows_sizes(rows, n)[0]
    named = sum(lengths) * spf
    for form in ("ptr", "rng"):
        results = []
        for fill, guard in M.FILLS:
            A = M.ArenaSet(dev, fill, guard)
            ws = A.scratch("workspace", n_ws)
            out = A.output("out_packed", torch.float32, (units.shape[0] * spf,))
            u_dev = A.input("unit_packed", units)
            nz = A.input("noise_packed", noise) if form == "ptr" else None
            for i in range(groups.shape[0]):
                sl = slice(i * rows, (i + 1) * rows)
                t_dev = A.input(f"table{i}", groups[i])
                g_dev = A.input(f"g{i}", torch.cat([g[owner[sl]], torch.zeros(rows - len(owner[sl]), g.shape[1])]))
                k_dev = A.input(f"keys{i}", torch.tensor(owner[sl] + [0] * (rows - len(owner[sl])), dtype=torch.int64))
                eng.infer_windows(ws, u_dev, nz, t_dev, g_dev, out, n, rng=None if form == "ptr" else (SEED, k_dev, 1.0))
            torch.cuda.synchronize()
            assert A.check() == [], (form, hex(fill), M.describe_guards(A.check()))
            assert A.changed_inputs() == [], (form, hex(fill))
            assert bool(torch.isfinite(out[:named]).all()), (form, hex(fill))
            results.append(out.clone())
            # (big, ...), (-1, -1, -1, 5) and (3, small, 0, 5) are idle after the clamp; (small, 21, small, big) clamps onto
            # the first window of utterance 0 and writes that row's own bits a second time
            assert bool((out[named:].reshape(-1).view(torch.uint8) == fill).all()), (form, hex(fill))
        for r in results[1:]:
            assert M.bits_equal(r[:named], results[0][:named]), form


# ---------------------------------------------------------------- the stated size
def test_shipped_config_bf16x(lib, dev):
    """The shipped config in bf16x, rows = 8, n = 256: one utterance of 2048 frames next to utterances of 40 and 300
    frames, generator form, each against qvc_infer_batch_ragged_rng of it alone."""
    import quickvc_official_amd as q
    from quickvc_official_amd.engine import QvcEngine
    from quickvc_official_amd.synth import make_synthetic_state_dict
    model = q.SynthesizerTrn(641, 32, **q.DEFAULT_MODEL_CONFIG)
    mc = dict(model.model_config, operand_dtype="bf16x")
    eng = QvcEngine(mc, make_synthetic_state_dict(model, 1234), dev)
    lengths, n, rows = (2048, 40, 300), 256, 8
    units, _noise, g = (t.to(dev) for t in packed_inputs(lengths, mc["inter_channels"], mc["gin_channels"], 9900))
    owner, keys = _owners(lengths, n), _keys(3)
    out = _launch(eng, units, table_rows(lengths, n), g[owner], n, rows, keys=[keys[u] for u in owner])
    spf = eng.samples_per_frame
    for u, (base, length) in enumerate(zip(_bases(lengths), lengths)):
        _check(out[base * spf:(base + length) * spf], _alone(eng, units, base, length, g[u], key=keys[u]), f"bf16x utterance {u} ({length} frames)")


# ---------------------------------------------------------------- Python surface and the CLI
def test_window_converter_and_infer_long_equal_infer(lib, dev):
    import quickvc_official_amd as q
    from quickvc_official_amd.windows import WindowConverter
    _mc, sd = mini_problem()
    net = q.SynthesizerTrn(641, 32, **q.MINI_MODEL_CONFIG)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    mc = net.model_config
    lengths = (70, 9, 150)
    units, noise, g = (t.to(dev) for t in packed_inputs(lengths, mc["inter_channels"], mc["gin_channels"], 9950))
    bases = _bases(lengths)
    us = [units[b:b + n] for b, n in zip(bases, lengths)]
    # generator form, graph replay, list input -- against infer_ragged of the list under the same (seed, keys)
    conv = WindowConverter(net, 4, 32, seed=5)
    got = conv.convert(us, g, keys=[11, 12, 13])
    want = net.infer_ragged([u.t() for u in us], g, seed=5, keys=[11, 12, 13])
    for u in range(3):
        _check(got[u], want[u].reshape(-1), f"WindowConverter rng utterance {u}")
    # pointer form, packed input, direct launches
    conv = WindowConverter(net, 4, 32, use_graph=False)
    got = conv.convert(units, g, noise=noise, lengths=lengths)
    want = net.infer_ragged([u.t() for u in us], g, noises=[noise[:, b:b + n] for b, n in zip(bases, lengths)])
    for u in range(3):
        _check(got[u], want[u].reshape(-1), f"WindowConverter ptr utterance {u}")
    # infer_long against infer on the whole
    unit = us[2].t().unsqueeze(0)
    nz = noise[:, bases[2]:bases[2] + lengths[2]].unsqueeze(0)
    _check(net.infer_long(unit, g[2:3], window_frames=32, rows=4, noise=nz), net.infer_batch(unit, g[2:3], nz), "infer_long ptr")
    _check(net.infer_long(unit, g[2:3], window_frames=32, rows=4, seed=5, key=3), net.infer_batch(unit, g[2:3], seed=5, keys=[3]), "infer_long rng")


def test_convert_cli_max_frames(lib, dev, tmp_path):
    """Three short sources and sources of 70 and 150 frames on the mini model: --noise native --max-frames 32 writes the
    files of the same run without the flag (>= 90 dB), with the pipeline's buffers sized by the short sources;
    --noise torch --max-frames 32 is refused by the parser."""
    from scipy.io import wavfile
    import quickvc_official_amd as q
    from quickvc_official_amd import convert as cli
    from quickvc_official_amd.checkpoint import save_checkpoint
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
    rs = np.random.RandomState(43)
    src_len = [31, 70, 24, 150, 27]
    for i, n in enumerate(src_len):
        np.save(str(tmp_path / f"u{i}.npy"), rs.randn(n, 256).astype(np.float32))
    items = [(f"o{i}", str(tmp_path / f"u{i}.npy"), str(tmp_path / f"spk{i % 2}.wav")) for i in range(len(src_len))]
    (tmp_path / "convert.txt").write_text("".join(f"{a}|{b}|{c}\n" for a, b, c in items))
    base = ["--hpfile", str(tmp_path / "config.json"), "--ptfile", str(tmp_path / "G_1.pth"), "--txtpath", str(tmp_path / "convert.txt"),
            "--seed", "5", "--io-threads", "2", "--batch", "4"]
    whole = cli.main(base + ["--noise", "native", "--outdir", str(tmp_path / "whole")])
    cut = cli.main(base + ["--noise", "native", "--max-frames", "32", "--outdir", str(tmp_path / "cut")])
    assert whole["utterances"] == cut["utterances"] == 5 and "windowed" not in whole
    assert cut["windowed"] == 2 and cut["pipeline_max_frames"] == 31
    for i, n in enumerate(src_len):
        _r, a = wavfile.read(str(tmp_path / "whole" / f"o{i}.wav"))
        _r, b = wavfile.read(str(tmp_path / "cut" / f"o{i}.wav"))
        assert a.shape == b.shape == (n * 320,)
        _check(torch.from_numpy(b.copy()), torch.from_numpy(a.copy()), f"--max-frames 32, source {i} ({n} frames)")
    with pytest.raises(SystemExit):
        cli.main(base + ["--noise", "torch", "--max-frames", "32", "--outdir", str(tmp_path / "bad")])
    with pytest.raises(SystemExit):
        cli.main(base + ["--max-frames", "32", "--outdir", str(tmp_path / "bad")])
