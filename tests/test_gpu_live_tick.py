"""The tick form of the windowed step on an MI355X (run with -m gpu): qvc_live_tick / _rng / _reset_slot through
QvcEngine and streaming.TickConverter -- per call, slot b brings n = clamp(n_new[b], 0, hop) frames, the counts in
device memory.  GPU output is compared with GPU output of the offline path (qvc_infer_batch_ragged[_rng]) at >= 90 dB,
the bar of tests/test_gpu_live.py, and the measured figure is printed; samples outside a stream and past n * spf must be
exact zeros.

  T1  the first n * spf samples of a tick's row are frames [pos - L, pos - L + n) of the offline conversion of the
      stream's first min(len, pos + n) frames (same g, same noise or the same (seed, key)); pos += n;
  T2  with L = C the concatenated output equals the whole-utterance conversion however the stream was cut;
  T3  with every n = hop each tick is torch.equal to LiveConverter.step on the same inputs;
  T4  a stream's output depends on its own slot alone.

NaN is placed wherever the contract says nothing is read: columns of unit_new / noise_new from n on, frames past a
stream's end, whole rows of idle slots, and the state before a slot is started.
"""
import ctypes
import functools
import random

import pytest
import torch

import config_space as CS
import memguard as M
import tick_patterns as TP
from helpers import load_case, regenerate, snr_db
import live_common as LC
from live_common import NAN, SEED, _Model, _debug_switches_at_defaults, _keys, dev, lib  # noqa: F401

pytestmark = pytest.mark.gpu

def _row_model(name, wn=None, dtype="f16"):
    return LC._row_model(name, wn, dtype, sizes="live_tick_sizes")


def _prefix_rows(eng, unit_b, g_b, noise_b, key, prefixes):
    return LC._prefix_rows(eng, unit_b, g_b, noise_b, key, prefixes, min_frames=2)


def _tick_inputs(unit, noise, at, n, lens, S, hop):
    """unit_new / noise_new of one tick: NaN everywhere but columns [0, n[s]) of the slots that bring frames of their
    stream (frames past a stream's end stay NaN too)."""
    u = torch.full((S, unit.shape[1], hop), NAN, device=unit.device)
    nz = None if noise is None else torch.full((S, noise.shape[1], hop), NAN, device=unit.device)
    for s in range(S):
        a, b = at[s], min(at[s] + n[s], lens[s])
        if b > a:
            u[s, :, :b - a] = unit[s, :, a:b]
            if nz is not None:
                nz[s, :, :b - a] = noise[s, :, a:b]
    return u, nz


def _tick_all(conv, unit, g, noise, lens, count_of, keys=None):
    """All slots started through start() on a state full of NaN bytes; ticks with n_new[s] = count_of(s, tick, hop) (raw:
    the library clamps) until every stream has flushed.  -> [(positions before, clamped counts, chunk)]"""
    S, hop = conv.streams, conv.hop
    conv._state.fill_(0xFF)
    for s in range(S):
        conv.start(s, g[s], length=lens[s], key=None if keys is None else keys[s])
    ticks, k = [], 0
    while not all(conv.finished(s) for s in range(S)):
        raw = [count_of(s, k, hop) for s in range(S)]
        at = [conv.position(s) for s in range(S)]
        u, nz = _tick_inputs(unit, noise, at, [TP.clamp(v, hop) for v in raw], lens, S, hop)
        out, n = conv.tick(u, raw, nz)
        assert n == [TP.clamp(v, hop) for v in raw] and [conv.position(s) for s in range(S)] == [a + c for a, c in zip(at, n)]
        ticks.append((at, n, out))
        k += 1
        assert k < 600
    assert conv._pos.tolist() == [conv.position(s) for s in range(S)], "the device positions and the host mirror disagree"
    return ticks


def _slot_ticks(ticks, slot):
    return [(at[slot], n[slot], out[slot]) for at, n, out in ticks]


def _check_stream(ticks, want_of_prefix, length, hop, L, spf, what=""):
    """One stream's ticks [(pos, n, row)] against want_of_prefix(prefix) (a 1-D waveform): zeros past n * spf and outside
    [0, length), the delivered frames concatenated and compared at 90 dB.  -> the concatenated waveform."""
    got, want = torch.full((length * spf,), NAN), torch.full((length * spf,), NAN)
    for at, n, row in ticks:
        row = row.cpu()
        assert bool((row[n * spf:] == 0).all()), (what, at, n, "not zero past n * spf")
        f0 = at - L
        lo, hi = max(f0, 0), min(f0 + n, length)
        inside = torch.zeros(hop * spf, dtype=torch.bool)
        if hi > lo:
            inside[(lo - f0) * spf:(hi - f0) * spf] = True
            got[lo * spf:hi * spf] = row[inside]
            want[lo * spf:hi * spf] = want_of_prefix(min(length, at + n))[lo * spf:hi * spf].cpu()
        head = row[:n * spf]
        assert bool((head[~inside[:n * spf]] == 0).all()), (what, at, n, "not zero outside the stream")
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(want).all()), what
    db = snr_db(want, got)
    print(f"{what} ({length} frames, {len(ticks)} ticks): {db:.1f} dB, bit-equal: {torch.equal(want, got)}")
    assert db >= 90.0, (what, db)
    return got


def _check_prefixes(eng, ticks, slot, unit_b, g_b, noise_b, key, length, hop, L, spf, what):
    """T1 for one stream: its ticks against the offline conversions of the prefixes it had reached."""
    mine = _slot_ticks(ticks, slot) if slot is not None else ticks
    prefixes = sorted({min(length, at + n) for at, n, _r in mine if n > 0 and at - L + n > 0 and at - L < length})
    rows = _prefix_rows(eng, unit_b, g_b, noise_b, key, prefixes)
    return _check_stream(mine, lambda p: rows[prefixes.index(p), 0], length, hop, L, spf, what)


# ---------------------------------------------------------------- T3 / T1 / graph: row wn_enc1_flow1, 23 / 9 / 16 frames, hop 7, L 4
T_LENS, T_HOP, T_L = [23, 9, 16], 7, 4


@functools.lru_cache(maxsize=None)
def _t_problem():
    from quickvc_official_amd.synth import make_synthetic_inputs
    model, C = _row_model("wn_enc1_flow1")
    mc = model.model_config
    unit, g, noise = make_synthetic_inputs(3, max(T_LENS), 256, mc["inter_channels"], mc["gin_channels"], seed0=8900)
    return model, C, unit.cuda(), g.cuda(), noise.cuda()


@pytest.mark.parametrize("trim", [1, 0], ids=["trimmed", "plain"])
@pytest.mark.parametrize("form", ["ptr", "rng"])
def test_lockstep_is_a_special_case(lib, dev, form, trim):
    """T3: every slot brings hop frames at every tick -- each tick's output is torch.equal to LiveConverter.step's on the
    same inputs, in both noise forms and both forms of the step, f16."""
    from quickvc_official_amd import lib as L
    from quickvc_official_amd.streaming import LiveConverter, TickConverter
    model, C, unit, g, noise = _t_problem()
    L.debug_set("live_trim", trim)                                        # read when the step is issued: at the captures
    seed = SEED if form == "rng" else None
    tick = TickConverter(model, 3, T_HOP, T_L, use_graph=True, seed=seed)
    live = LiveConverter(model, 3, T_HOP, T_L, use_graph=True, seed=seed)
    assert tick.window == live.window == C + T_L + T_HOP == 46 and tick.lag == T_L
    for conv in (tick, live):
        conv._state.fill_(0xFF)
        for s in range(3):
            conv.start(s, g[s], length=T_LENS[s], key=_keys(3)[s])
    k = 0
    while not all(live.finished(s) for s in range(3)):
        at = [live.position(s) for s in range(3)]
        assert at == [tick.position(s) for s in range(3)] == [k * T_HOP] * 3
        u, nz = _tick_inputs(unit, noise if form == "ptr" else None, at, [T_HOP] * 3, T_LENS, 3, T_HOP)
        want = live.step(u, nz)
        got, n = tick.tick(u, [T_HOP] * 3, nz)
        assert n == [T_HOP] * 3 and bool(torch.isfinite(want).all())
        assert torch.equal(got, want), (form, trim, k, "the tick with n = hop differs from the lockstep step")
        k += 1
    assert k == -(-(max(T_LENS) + T_L) // T_HOP) and all(tick.finished(s) for s in range(3))


@pytest.mark.parametrize("form", ["rng", "ptr"])
def test_prefix_exactness(lib, dev, form):
    """T1 with the fixed pattern of tests/tick_patterns.py at hop 7 (W = 35 + 4 + 7 = 46): ticks of 0, 1, 2, 3 and 7 frames
    (shifts that are 4-byte aligned only), -3 and 12, n = 0 at the first tick, n = 1 at pos 0, idle runs of three ticks,
    the stream ends inside ticks, flush ticks.  Graph replay."""
    from quickvc_official_amd.streaming import TickConverter
    model, _C, unit, g, noise = _t_problem()
    eng, spf = model.engine(), model.samples_per_frame
    conv = TickConverter(model, 3, T_HOP, T_L, use_graph=True, seed=SEED if form == "rng" else None)
    assert (conv._rng_graph if form == "rng" else conv._graph) is not None
    nz = None if form == "rng" else noise
    ticks = _tick_all(conv, unit, g, nz, T_LENS, TP.raw_count, keys=_keys(3))
    seen = {n for _a, ns, _o in ticks for n in ns}
    assert {0, 1, 2, 3, T_HOP} <= seen and ticks[0][1][0] == 0 and ticks[0][1][1] == 1 and ticks[1][0][0] == 0 and ticks[1][1][0] == 1
    for b, length in enumerate(T_LENS):
        _check_prefixes(eng, ticks, b, unit[b], g[b], None if nz is None else nz[b], _keys(3)[b], length, T_HOP, T_L, spf, f"T1 {form} slot {b}")


def test_graph_replay_equals_direct_launches(lib, dev):
    """The same streams and the same pattern with use_graph True and False: torch.equal at every tick."""
    from quickvc_official_amd.streaming import TickConverter
    model, _C, unit, g, _noise = _t_problem()
    runs = []
    for graph in (True, False):
        conv = TickConverter(model, 3, T_HOP, T_L, use_graph=graph, seed=SEED)
        assert (conv._rng_graph is not None) == graph
        runs.append(_tick_all(conv, unit, g, None, T_LENS, TP.raw_count, keys=_keys(3)))
    assert len(runs[0]) == len(runs[1])
    for (a0, n0, o0), (a1, n1, o1) in zip(*runs):
        assert a0 == a1 and n0 == n1 and torch.equal(o0, o1)


# ---------------------------------------------------------------- T2
def _random_cut(rng, hop):
    """count_of for one stream: seeded counts in [0, hop]; the first two ticks are a 0 and a hop, so both occur."""
    memo = {}

    def count_of(_slot, k, _hop):
        if k not in memo:
            memo[k] = 0 if k == 0 else (hop if k == 1 else rng.randint(0, hop))
        return memo[k]
    return count_of


@pytest.mark.parametrize("name", ["one_up8", "istft_ups3", "mb_up16_up1"])
def test_chunking_invariance_at_full_look_ahead(lib, dev, name):
    """T2: L = C at hop 5 on one up-sampler, the single-band decoder with three up-samplers and the multiband decoder
    (WaveNet (2, 1, 2) keeps W small, as in tests/test_gpu_live.py).  Streams of T = W + 3 * hop + 1 and T // 3 frames, two
    seeded cuts per stream with counts in [0, hop]: both equal the whole-utterance conversion, and each other."""
    from quickvc_official_amd.streaming import TickConverter
    from quickvc_official_amd.synth import make_synthetic_inputs
    model, C = _row_model(name, wn=(2, 1, 2))
    mc, eng, spf = model.model_config, model.engine(), model.samples_per_frame
    hop = 5
    conv = TickConverter(model, 2, hop, C, use_graph=True, seed=SEED)
    assert conv.window == 2 * C + hop
    T = conv.window + 3 * hop + 1
    lens = [T, T // 3]
    unit, g, _n = make_synthetic_inputs(2, T, 256, mc["inter_channels"], mc["gin_channels"], seed0=9000)
    unit, g = unit.cuda(), g.cuda()
    keys = _keys(2)
    whole = eng.infer_batch_ragged(unit, g, None, torch.tensor(lens, dtype=torch.int32), rng=(SEED, keys, 1.0)).clone()
    cuts = []
    for c in range(2):
        per_slot = [_random_cut(random.Random(9100 + 10 * c + s), hop) for s in range(2)]
        ticks = _tick_all(conv, unit, g, None, lens, lambda s, k, h: per_slot[s](s, k, h), keys=keys)
        for s in range(2):
            counts = [n[s] for _a, n, _o in ticks]
            assert 0 in counts and hop in counts and all(0 <= v <= hop for v in counts)
        cuts.append([_check_stream(_slot_ticks(ticks, s), lambda p, s=s: whole[s, 0], lens[s], hop, C, spf, f"{name} C={C} cut {c} slot {s}")
                     for s in range(2)])
    for s in range(2):
        db = snr_db(cuts[0][s], cuts[1][s])
        print(f"{name} slot {s}: cut 0 against cut 1 {db:.1f} dB")
        assert db >= 90.0, (name, s, db)


# ---------------------------------------------------------------- T4
def test_slots_tick_independently(lib, dev):
    """T4: five streams of 40 / 13 / 29 / 7 / 22 frames through two slots at hop 6, L = 3, graph replay.  A stream is
    admitted with start() when a slot frees up and ticks by its own seeded pattern; a slot that is not ticking is sent
    NaN rows.  Every stream is compared with ITS OWN prefix conversions."""
    from quickvc_official_amd.streaming import TickConverter
    from quickvc_official_amd.synth import make_synthetic_inputs
    model, _C = _row_model("wn_enc1_flow1")
    mc, eng, spf = model.model_config, model.engine(), model.samples_per_frame
    lens, S, hop, L = [40, 13, 29, 7, 22], 2, 6, 3
    N = len(lens)
    unit, g, _n = make_synthetic_inputs(N, max(lens), 256, mc["inter_channels"], mc["gin_channels"], seed0=9200)
    unit, g = unit.cuda(), g.cuda()
    keys = _keys(N)
    conv = TickConverter(model, S, hop, L, use_graph=True, seed=SEED)
    conv.reset(lengths=torch.zeros(S, dtype=torch.int32))                  # every slot idle
    conv._state.fill_(0xFF)
    pattern = [random.Random(9300 + i) for i in range(N)]
    occupant, log = [None] * S, {i: [] for i in range(N)}
    nxt, done, n_ticks, admitted_at = 0, 0, 0, {}
    while done < N:
        for s in range(S):
            if occupant[s] is None and nxt < N:
                conv.start(s, g[nxt], length=lens[nxt], key=keys[nxt])
                occupant[s], admitted_at[nxt] = nxt, n_ticks
                nxt += 1
        raw = [0 if i is None else pattern[i].choice([0, 0, 1, 2, 3, hop, hop, hop + 2]) for i in occupant]
        n = [TP.clamp(v, hop) for v in raw]
        u = torch.full((S, 256, hop), NAN, device=dev)
        at = [conv.position(s) for s in range(S)]
        for s, i in enumerate(occupant):
            if i is not None:
                a, b = at[s], min(at[s] + n[s], lens[i])
                if b > a:
                    u[s, :, :b - a] = unit[i, :, a:b]
        out, got_n = conv.tick(u, raw)
        assert got_n == n
        n_ticks += 1
        for s, i in enumerate(occupant):
            if i is None:
                assert bool((out[s] == 0).all())
                continue
            log[i].append((at[s], n[s], out[s].clone()))
            if conv.finished(s):
                occupant[s], done = None, done + 1
        assert n_ticks < 400
    assert len(set(admitted_at.values())) >= 3
    for i, length in enumerate(lens):
        _check_prefixes(eng, log[i], None, unit[i], g[i], None, keys[i], length, hop, L, spf, f"T4 stream {i} admitted at tick {admitted_at[i]}")


# ---------------------------------------------------------------- the stated size
def test_ticks_at_stated_size(lib, dev):
    """The shipped config, 64 streams, hop 16, L = 8, `bf16x`, one graph replay per tick, 8 ticks.  In every tick a seeded
    third of the slots is idle, a third brings 16 frames and a third 1-15.  Finite everywhere, slots 0 / 21 / 63 against
    their prefix conversions, all positions equal to the sums of their counts."""
    import quickvc_official_amd as q
    from quickvc_official_amd.streaming import TickConverter
    from quickvc_official_amd.synth import make_synthetic_inputs
    entry, _ = load_case("full_b1")
    _m, sd, _u, _g, _n = regenerate(entry)
    model = q.SynthesizerTrn(641, 32, **dict(entry["config"], operand_dtype="bf16x"))
    model.load_state_dict(sd)
    model = model.cuda().eval()
    S, hop, L, n_ticks = 64, 16, 8, 8
    unit, g, noise = make_synthetic_inputs(S, hop * n_ticks, 256, 192, 256, seed0=9400)
    unit, g, noise = unit.cuda(), g.cuda(), noise.cuda()
    conv = TickConverter(model, S, hop, L, use_graph=True)
    assert conv._graph is not None and conv.window == conv.context + L + hop
    conv.reset(g)
    eng, spf = model.engine(), model.samples_per_frame
    rnd = random.Random(9500)
    lens = [2 ** 30] * S
    ticks, sums = [], [0] * S
    for _k in range(n_ticks):
        order = list(range(S))
        rnd.shuffle(order)
        n = [0] * S
        for j, s in enumerate(order):
            n[s] = 0 if j < S // 3 else (hop if j < 2 * (S // 3) else rnd.randint(1, hop - 1))
        at = [conv.position(s) for s in range(S)]
        assert at == sums
        u, nz = _tick_inputs(unit, noise, at, n, lens, S, hop)
        out, got_n = conv.tick(u, n, nz)
        assert got_n == n and out.shape == (S, hop * spf) and bool(torch.isfinite(out).all())
        ticks.append((at, n, out))
        sums = [a + c for a, c in zip(sums, n)]
    assert conv._pos.tolist() == sums == [conv.position(s) for s in range(S)]
    for s in (0, 21, 63):
        mine = _slot_ticks(ticks, s)
        delivered = max(at + n - L for at, n, _r in mine)
        assert delivered > 0, s
        # the stream has not ended: compare the frames delivered so far
        prefixes = sorted({at + n for at, n, _r in mine if n > 0 and at - L + n > 0})
        rows = _prefix_rows(eng, unit[s], g[s], noise[s], None, prefixes)
        got, want = [], []
        for at, n, row in mine:
            assert bool((row[n * spf:] == 0).all())
            f0 = at - L
            lo, hi = max(f0, 0), f0 + n
            assert bool((row[:max(lo - f0, 0) * spf] == 0).all())
            if hi > lo:
                got.append(row[(lo - f0) * spf:n * spf].cpu())
                want.append(rows[prefixes.index(at + n), 0, lo * spf:hi * spf].cpu())
        db = snr_db(torch.cat(want), torch.cat(got))
        print(f"stated size slot {s}: {sum(t.numel() for t in got) // spf} frames delivered, {db:.1f} dB")
        assert db >= 90.0, (s, db)


# ---------------------------------------------------------------- memory contract
def _ptr(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("form", ["ptr", "rng"])
def test_memory_contract(lib, dev, form):
    """Every qvc_live_tick[_rng] of the T1 streams (23 / 9 / 16 frames, hop 7, L = 4, row wn_enc1_flow1) under the fixed
    pattern to the flush, raw C ABI, every caller-owned buffer in a guarded arena (tests/memguard.py) of exactly the
    queried size.  state, workspace (stale from tick to tick), out, pos_dev and len_dev start from the fill (0x00 / 0x3C /
    0xFF = NaN) and the slots are started by qvc_live_tick_reset_slot; n_new_dev, len_dev's source, g, unit_new, noise_new
    and the blob are tracked inputs.  Guards intact, inputs unchanged, pos advanced by the clamped counts, zeros where the
    contract says so, outputs bit-equal across the fills and equal to TickConverter's."""
    from quickvc_official_amd import lib as L
    from quickvc_official_amd.streaming import TickConverter
    model, _C, unit_d, g_d, noise_d = _t_problem()
    eng = model.engine()
    mc = model.model_config
    cfgp = ctypes.byref(eng.cfg)
    lens, hop, L_ = T_LENS, T_HOP, T_L
    S_, UC, C_in, spf = 3, 256, mc["inter_channels"], model.samples_per_frame
    unit, g, noise = unit_d.cpu(), g_d.cpu(), noise_d.cpu()
    n_state, n_ws = int(lib.qvc_live_tick_state_bytes(cfgp, S_, hop, L_)), int(lib.qvc_live_tick_workspace_bytes(cfgp, S_, hop, L_))
    assert n_state > 0 and n_ws > 0
    keys = torch.tensor([k - (1 << 64) if k >> 63 else k for k in _keys(S_)], dtype=torch.int64)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    results = []
    for fill, guard in M.FILLS:
        A = M.ArenaSet(dev, fill, guard)
        junk = NAN if fill == 0xFF else 123.0
        bl, gg = A.input("blob", eng.blob.cpu()), A.input("g", g)
        kd = A.input("keys_dev", keys)
        ld = A.input("len_dev", torch.tensor(lens, dtype=torch.int32))
        state, ws = A.scratch("state", n_state), A.scratch("workspace", n_ws)
        out = A.output("out", torch.float32, (S_, hop * spf))
        pos, ln_reset = A.output("pos_dev", torch.int32, (S_,)), A.output("len_reset", torch.int32, (S_,))
        for b, n in enumerate(lens):
            assert lib.qvc_live_tick_reset_slot(cfgp, _ptr(state), n_state, S_, hop, L_, b, n, _ptr(pos), _ptr(ln_reset), stream()) == 0
        torch.cuda.synchronize()
        assert pos.tolist() == [0] * S_ and ln_reset.tolist() == lens
        rng = L.QvcNoiseRng(SEED, _ptr(kd), 1.0)
        log, at, k = [], [0] * S_, 0
        while any(at[b] - L_ < lens[b] for b in range(S_)):
            raw = [TP.raw_count(b, k, hop) for b in range(S_)]
            n = [TP.clamp(v, hop) for v in raw]
            u_new, z_new = torch.full((S_, UC, hop), junk), torch.full((S_, C_in, hop), junk)
            for b, end in enumerate(lens):
                hi = min(at[b] + n[b], end)
                if hi > at[b]:
                    u_new[b, :, :hi - at[b]] = unit[b, :, at[b]:hi]
                    z_new[b, :, :hi - at[b]] = noise[b, :, at[b]:hi]
            ud, nd = A.input("unit_new", u_new), A.input("noise_new", z_new)
            cd = A.input("n_new_dev", torch.tensor(raw, dtype=torch.int32))
            out.view(torch.uint8).fill_(fill)
            if form == "ptr":
                st = lib.qvc_live_tick(cfgp, _ptr(bl), _ptr(state), n_state, _ptr(ud), _ptr(gg), _ptr(nd), _ptr(out), S_, hop, L_,
                                       _ptr(cd), _ptr(pos), _ptr(ld), _ptr(ws), n_ws, stream())
            else:
                st = lib.qvc_live_tick_rng(cfgp, _ptr(bl), _ptr(state), n_state, _ptr(ud), _ptr(gg), ctypes.byref(rng), _ptr(out), S_, hop, L_,
                                           _ptr(cd), _ptr(pos), _ptr(ld), _ptr(ws), n_ws, stream())
            torch.cuda.synchronize()
            assert st == 0, (hex(fill), k, st)
            assert A.changed_inputs() == [], (hex(fill), k)
            log.append((list(at), n, out.clone()))
            at = [a + c for a, c in zip(at, n)]
            assert pos.tolist() == at, (hex(fill), k)
            k += 1
            assert k < 200
        damaged = A.check()
        assert not damaged, f"fill {fill:#x}: {M.describe_guards(damaged)}"
        for a_, n_, o_ in log:
            for b, end in enumerate(lens):
                assert bool((o_[b, n_[b] * spf:] == 0).all()), (hex(fill), a_, b)
                f0 = a_[b] - L_
                lo, hi = max(f0, 0), min(f0 + n_[b], end)
                head = o_[b, :n_[b] * spf]
                inside = torch.zeros(n_[b] * spf, dtype=torch.bool, device=dev)
                if hi > lo:
                    inside[(lo - f0) * spf:(hi - f0) * spf] = True
                assert bool((head[~inside] == 0).all()) and bool(torch.isfinite(head).all()), (hex(fill), a_, b)
        results.append(log)
    for (fill, _g), res in zip(M.FILLS[1:], results[1:]):
        assert len(res) == len(results[0])
        for (a0, n0, o0), (a1, n1, o1) in zip(results[0], res):
            assert a0 == a1 and n0 == n1
            assert M.bits_equal(o0, o1), f"the output depends on what the buffers held: fill {fill:#x} differs from fill 0x0"
    conv = TickConverter(model, S_, hop, L_, use_graph=False, seed=SEED if form == "rng" else None)
    ticks = _tick_all(conv, unit_d, g_d, None if form == "rng" else noise_d, lens, TP.raw_count, keys=_keys(S_))
    assert len(ticks) == len(results[0])
    for (a0, n0, o0), (a1, n1, o1) in zip(results[0], ticks):
        assert a0 == a1 and n0 == n1 and torch.equal(o0, o1), "the raw ABI run differs from TickConverter's"
