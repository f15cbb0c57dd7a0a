"""The tick form of the segment rings on an MI355X (run with -m gpu): qvc_stream_tick / _rng through the raw C ABI,
QvcEngine and streaming.StreamTickConverter -- per call, slot b brings n = clamp(n_new[b], 0, hop) frames, the counts in
device memory, on qvc_stream_step's state.  GPU output is compared with GPU output of the offline path
(qvc_infer_batch_ragged[_rng] on the whole utterance, same g, same noise or (seed, key)) at >= 90 dB, the project's
streaming bar; the measured figure and whether the two are bit-equal are printed.  Properties S1 - S6 and the shapes are
those of tests/test_stream_tick_host.py (the loop and the per-tick checks are shared: tests/stream_tick_common.py), in both
forms of the noise; added here: one captured graph for any pattern, the stated size, the memory contract, and the
status codes on real device buffers.

NaN is placed wherever the contract says nothing is read: columns of unit_new / noise_new from n on, frames past a
stream's end, whole rows of idle slots, and the state and workspace before a slot is started.
"""
import ctypes
import functools

import pytest
import torch

import memguard as M
import stream_tick_common as SC
import tick_patterns as TP
from helpers import load_case, regenerate
from live_common import SEED, _Model, _debug_switches_at_defaults, _keys, dev, lib, twin_library  # noqa: F401
from stream_tick_common import LENS, NAN, ROW, ROW_MB

pytestmark = pytest.mark.gpu
S = len(LENS)


@functools.lru_cache(maxsize=None)
def _model(name):
    mc, sd = SC.row_problem(name)
    return _Model(mc, sd, torch.device("cuda:0"))


@functools.lru_cache(maxsize=None)
def _twin():
    return SC.declare_twin(twin_library())       # host arithmetic only: the ring table


def _ptr(t):
    return None if t is None else t.data_ptr()


class GpuRunner:
    """stream_tick_common's runner surface over the raw C ABI.  Buffers come from `arenas` (a memguard.ArenaSet: exactly
    the queried sizes between guards, filled with its fill) or are plain tensors filled with 0xFF."""

    def __init__(self, lib, name, hop, form, arenas=None):
        from quickvc_official_amd import lib as L
        from quickvc_official_amd.engine import aligned_empty
        model = _model(name)
        self.eng, self.lib, self.form, self.B, self.hop, self.A = model.engine(), lib, form, S, hop, arenas
        eng, d = self.eng, self.eng.device
        self.p = ctypes.byref(eng.cfg)
        self.n_state, self.n_ws, self.lag, self.nlag = eng.stream_tick_sizes(S, hop)
        self.n_ws_step = eng.stream_sizes(S, hop)[1]
        assert self.n_ws > self.n_ws_step and self.n_state == eng.stream_sizes(S, hop)[0]
        self.spf = model.samples_per_frame
        _unit, g, _noise = SC.row_inputs(name)
        keys = torch.tensor([k - (1 << 64) if k >> 63 else k for k in _keys(S)], dtype=torch.int64)
        if arenas is None:
            self._state, self._ws = aligned_empty(self.n_state, d).fill_(0xFF), aligned_empty(self.n_ws, d).fill_(0xFF)
            self._out = torch.empty(S, hop * self.spf, device=d)
            self._pos, self._len = torch.full((S,), 12345, dtype=torch.int32, device=d), torch.full((S,), -7, dtype=torch.int32, device=d)
            self.g, self._keys, self.blob = g.to(d), keys.to(d), eng.blob
        else:
            self._state, self._ws = arenas.scratch("state", self.n_state), arenas.scratch("workspace", self.n_ws)
            self._out = arenas.output("out", torch.float32, (S, hop * self.spf))
            self._pos, self._len = arenas.output("pos_dev", torch.int32, (S,)), arenas.output("len_dev", torch.int32, (S,))
            self.g, self._keys, self.blob = arenas.input("g", g), arenas.input("keys_dev", keys), arenas.input("blob", eng.blob.cpu())
        self.rng = L.QvcNoiseRng(SEED, _ptr(self._keys), 1.0)
        self.table = SC.ring_table(_twin(), eng.cfg, S, hop)
        assert sum(n for per in self.table for _o, n, _r, _k, _h in per) <= self.n_state

    def _stream(self):
        return torch.cuda.current_stream().cuda_stream

    def reset_slot(self, b, length):
        st = self.lib.qvc_stream_reset_slot(self.p, _ptr(self._state), self.n_state, self.B, self.hop, b, int(length), _ptr(self._pos),
                                            _ptr(self._len), self._stream())
        assert st == 0, st

    def state(self):
        return self._state.cpu()

    def positions(self):
        return self._pos.tolist()

    def _put(self, name, host):
        return host.to(self.eng.device) if self.A is None else self.A.input(name, host)

    def _call(self, tick, u_new, z_new, raw):
        u, z = self._put("unit_new", u_new), self._put("noise_new", z_new)
        if self.A is not None:
            self._out.view(torch.uint8).fill_(self.A.fill)
        else:
            self._out.fill_(NAN)
        stem = "qvc_stream_tick" if tick else "qvc_stream_step"
        fn, draw = (getattr(self.lib, stem), _ptr(z)) if self.form == "ptr" else (getattr(self.lib, stem + "_rng"), ctypes.byref(self.rng))
        head = (self.p, _ptr(self.blob), _ptr(self._state), self.n_state, _ptr(u), _ptr(self.g), draw, _ptr(self._out), self.B, self.hop)
        if tick:
            cd = self._put("n_new_dev", torch.tensor(raw, dtype=torch.int32))
            st = fn(*head, _ptr(cd), _ptr(self._pos), _ptr(self._len), _ptr(self._ws), self.n_ws, self._stream())
        else:
            st = fn(*head, _ptr(self._pos), _ptr(self._len), _ptr(self._ws), self.n_ws_step, self._stream())
        torch.cuda.synchronize()
        assert st == 0, (stem, st)
        if tick:
            assert cd.tolist() == list(raw), "n_new_dev was written"
        if self.A is not None:
            assert self.A.changed_inputs() == [], self.A.changed_inputs()
        return self._out.clone()

    def tick(self, u_new, z_new, raw):
        return self._call(True, u_new, z_new, raw)

    def step(self, u_new, z_new):
        out = self._call(False, u_new, z_new, None)
        self._pos += self.hop
        return out


@functools.lru_cache(maxsize=None)
def _whole(name, form):
    """The GPU's whole-utterance conversion of the row's three streams; computed once, read-only."""
    eng = _model(name).engine()
    unit, g, noise = (t.cuda() for t in SC.row_inputs(name))
    frames = torch.tensor(LENS, dtype=torch.int32)
    if form == "ptr":
        return eng.infer_batch_ragged(unit, g, noise, frames).clone().cpu()
    return eng.infer_batch_ragged(unit, g, None, frames, rng=(SEED, _keys(S), 1.0)).clone().cpu()


@functools.lru_cache(maxsize=None)
def _cut(name, hop, form, which):
    """The ticks of the row's streams cut by `which`; computed once, read-only."""
    from quickvc_official_amd import lib as L
    unit, _g, noise = SC.row_inputs(name)
    R = GpuRunner(L.load_library(), name, hop, form)
    seen = set()

    def count_of(b, k, h):
        v = {"pattern": TP.raw_count, "ones": TP.all_one, "full": TP.all_hop}[which](b, k, h)
        seen.add(v)
        return v
    return R, SC.run_streams(R, unit, noise, LENS, count_of), seen


# ---------------------------------------------------------------- S1
@pytest.mark.parametrize("name,hop,form", [(ROW, 4, "ptr"), (ROW, 5, "rng"), (ROW_MB, 5, "ptr")])
def test_lockstep_is_the_special_case(lib, dev, name, hop, form):
    """S1: after EVERY call out is torch.equal to qvc_stream_step's and so is the kept part of every row of every ring of
    every slot; a third state on which the two calls alternate gives the same outputs."""
    unit, _g, noise = SC.row_inputs(name)
    runs = {}
    for key, call in (("step", lambda k: "step"), ("tick", None), ("mixed", lambda k: "step" if k % 2 else "tick")):
        R, states = GpuRunner(lib, name, hop, form), []
        ticks = SC.run_streams(R, unit, noise, LENS, TP.all_hop, call=call,
                               between=lambda k, R_, at: (states.append(R_.state()) if k else None) or at)
        states.append(R.state())
        runs[key] = (R, ticks, states)
    (sR, st_t, st_s), (tR, tk_t, tk_s), (_mR, mx_t, _ms) = runs["step"], runs["tick"], runs["mixed"]
    assert len(st_t) == len(tk_t) == len(mx_t) == -(-(max(LENS) + sR.lag) // hop)
    for k in range(len(st_t)):
        assert bool(torch.isfinite(st_t[k][2]).all())
        assert torch.equal(tk_t[k][2], st_t[k][2]), (k, "the tick with n = hop differs from the lockstep step")
        assert torch.equal(mx_t[k][2], st_t[k][2]), (k, "alternating step and tick on one state differs from lockstep alone")
        for b in range(S):
            assert torch.equal(SC.kept_bytes(tk_s[k], tR.table, b), SC.kept_bytes(st_s[k], sR.table, b)), (k, b, "ring bytes differ")


# ---------------------------------------------------------------- S2
@pytest.mark.parametrize("name,hop,form", [(ROW, 4, "ptr"), (ROW, 4, "rng"), (ROW, 5, "ptr"), (ROW, 5, "rng"), (ROW_MB, 4, "rng")])
def test_exactness_under_the_pattern(lib, dev, name, hop, form):
    R, ticks, seen = _cut(name, hop, form, "pattern")
    SC.check_pattern_holds(ticks, LENS, hop, seen)
    whole = _whole(name, form)
    for b, length in enumerate(LENS):
        got = SC.collect(ticks, b, length, R.lag, R.spf, f"{name} hop {hop} {form}")
        SC.compare(whole[b, 0, :length * R.spf], got, f"{name} hop {hop} {form} slot {b} ({length} frames, {len(ticks)} ticks) against the whole utterance")


# ---------------------------------------------------------------- S3
@pytest.mark.parametrize("hop,form", [(4, "rng"), (5, "ptr")])
def test_independence_of_the_cut(lib, dev, hop, form):
    cuts = {}
    for which in ("pattern", "ones", "full"):
        R, ticks, _seen = _cut(ROW, hop, form, which)
        cuts[which] = [SC.collect(ticks, b, length, R.lag, R.spf, which) for b, length in enumerate(LENS)]
    for x, y in (("pattern", "ones"), ("pattern", "full"), ("ones", "full")):
        for b in range(S):
            SC.compare(cuts[x][b], cuts[y][b], f"hop {hop} {form} slot {b}: cut '{x}' against cut '{y}'")


# ---------------------------------------------------------------- S4
@pytest.mark.parametrize("hop,form", [(4, "ptr"), (5, "ptr"), (5, "rng")])
def test_unused_columns_are_never_read(lib, dev, hop, form):
    """The pattern's run feeds NaN in columns [n, hop), in the whole rows of idle slots and past a stream's end; the same
    run with 0.25 there is torch.equal, and finite."""
    unit, _g, noise = SC.row_inputs(ROW)
    _R, nan_ticks, _seen = _cut(ROW, hop, form, "pattern")
    clean = SC.run_streams(GpuRunner(lib, ROW, hop, form), unit, noise, LENS, TP.raw_count, junk=0.25)
    assert len(clean) == len(nan_ticks)
    for (a0, n0, o0), (a1, n1, o1) in zip(nan_ticks, clean):
        assert a0 == a1 and n0 == n1 and bool(torch.isfinite(o0).all()) and torch.equal(o0, o1), a0


# ---------------------------------------------------------------- S5 / S6
def test_idle_ticks_occur_and_leave_no_trace(lib, dev):
    """S5 is asserted inside run_streams at every tick (state bytes by slot_range over the ring table, pos); here: the
    pattern's run did hold idle ticks of every slot, at pos 0 and mid-stream, and the idle rows of `out` are zeros."""
    _R, ticks, _seen = _cut(ROW, 5, "ptr", "pattern")
    for b in range(S):
        idle = [(at[b], out[b]) for at, n, out in ticks if n[b] == 0]
        assert len(idle) >= 3 and any(a > 0 for a, _o in idle), b
        assert all(bool((o == 0).all()) for _a, o in idle)


@pytest.mark.parametrize("hop,form", [(4, "rng"), (5, "ptr")])
def test_slots_tick_independently(lib, dev, hop, form):
    """S6: slot 1's outputs, tick by tick, with its neighbours ticking by the pattern, idle throughout, and re-admitted
    with qvc_stream_reset_slot mid-stream (slot 0 at tick 5, slot 2 at ticks 3 and 9)."""
    unit, _g, noise = SC.row_inputs(ROW)
    _R, base, _seen = _cut(ROW, hop, form, "pattern")

    def alone(b, k, h):
        return TP.raw_count(b, k, h) if b == 1 else 0

    def readmit(k, R, at):
        at = list(at)
        for slot, when in ((0, (5,)), (2, (3, 9))):
            if k in when:
                R.reset_slot(slot, LENS[slot])
                at[slot] = 0
        return at
    runs = [SC.run_streams(GpuRunner(lib, ROW, hop, form), unit, noise, LENS, alone, watch=[1]),
            SC.run_streams(GpuRunner(lib, ROW, hop, form), unit, noise, LENS, TP.raw_count, watch=[1], between=readmit)]
    for ticks in runs:
        assert 0 < len(ticks) <= len(base)
        for (a0, n0, o0), (a1, n1, o1) in zip(base, ticks):
            assert a0[1] == a1[1] and n0[1] == n1[1] and torch.equal(o0[1], o1[1]), (hop, a0)


# ---------------------------------------------------------------- one graph, any pattern
def _convert_by_pattern(conv, unit, g, noise, keys):
    """The row's streams through StreamTickConverter.tick under the fixed pattern -> [(positions, counts, out on the host)]."""
    hop = conv.hop
    conv._state.fill_(0xFF)
    for s in range(S):
        conv.start(s, g[s], length=LENS[s], key=keys[s])
    ticks, k = [], 0
    while not all(conv.finished(s) for s in range(S)):
        raw = [TP.raw_count(s, k, hop) for s in range(S)]
        at = [conv.position(s) for s in range(S)]
        u, z = SC.tick_inputs(unit, noise, at, [TP.clamp(v, hop) for v in raw], LENS, hop, conv.noise_lag)
        out, n = conv.tick(u.cuda(), raw, None if conv._rng is not None else z.cuda())
        assert n == [TP.clamp(v, hop) for v in raw]
        ticks.append((at, n, out.cpu()))
        k += 1
        assert k < 400
    assert conv._pos.tolist() == [conv.position(s) for s in range(S)], "the device positions and the host mirror disagree"
    return ticks


@pytest.mark.parametrize("hop,form", [(5, "rng"), (4, "ptr")])
def test_one_graph_serves_any_pattern(lib, dev, hop, form):
    """ONE capture of the call (StreamTickConverter's) replayed with the pattern's counts is torch.equal, tick by tick, to
    direct launches through the converter and through the raw C ABI."""
    from quickvc_official_amd.streaming import StreamTickConverter
    model = _model(ROW)
    unit, g, noise = SC.row_inputs(ROW)
    runs = []
    for graph in (True, False):
        conv = StreamTickConverter(model, S, hop, use_graph=graph, seed=SEED if form == "rng" else None)
        assert ((conv._rng_graph if form == "rng" else conv._graph) is not None) == graph
        runs.append(_convert_by_pattern(conv, unit, g.cuda(), noise, _keys(S)))
    _R, raw_ticks, _seen = _cut(ROW, hop, form, "pattern")
    assert len(runs[0]) == len(runs[1]) == len(raw_ticks)
    for (a0, n0, o0), (a1, n1, o1), (a2, n2, o2) in zip(runs[0], runs[1], raw_ticks):
        assert a0 == a1 == a2 and n0 == n1 == n2
        assert torch.equal(o0, o1), (a0, "graph replay differs from direct launches")
        assert torch.equal(o0, o2), (a0, "the converter differs from the raw C ABI")


def test_step_of_the_tick_converter_is_the_stream_converter(lib, dev):
    """StreamTickConverter.convert (step = the tick with every n = hop) is torch.equal to StreamConverter.convert."""
    from quickvc_official_amd.streaming import StreamConverter, StreamTickConverter
    model = _model(ROW)
    unit, g, noise = (t.cuda() for t in SC.row_inputs(ROW))
    lens = torch.tensor(LENS, dtype=torch.int32)
    want = StreamConverter(model, S, 5).convert(unit, g, noise, lengths=lens)
    got = StreamTickConverter(model, S, 5).convert(unit, g, noise, lengths=lens)
    assert bool(torch.isfinite(want).all()) and torch.equal(got, want)


# ---------------------------------------------------------------- the stated size
def test_ticks_at_stated_size(lib, dev):
    """The shipped geometry, 64 slots, hop 16, bf16x, one graph replay per tick, the fixed pattern over the slots, until
    probe slots 0 and 37 have delivered 32 frames each: those against the offline conversion of what the probe was fed
    (the streams have not ended; the delivered frames lie more than the receptive field in front of that end)."""
    import quickvc_official_amd as q
    from quickvc_official_amd.streaming import StreamTickConverter
    from quickvc_official_amd.synth import make_synthetic_inputs
    entry, _ = load_case("full_b1")
    _m, sd, _u, _g, _n = regenerate(entry)
    model = q.SynthesizerTrn(641, 32, **dict(entry["config"], operand_dtype="bf16x"))
    model.load_state_dict(sd)
    model = model.cuda().eval()
    B, hop, want_frames, probes = 64, 16, 32, (0, 37)
    conv = StreamTickConverter(model, B, hop, use_graph=True)
    assert conv._graph is not None
    lag, nlag, spf = conv.lag, conv.noise_lag, conv.spf
    T = 12 * hop + lag + want_frames
    unit, g, noise = make_synthetic_inputs(B, T, 256, 192, 256, seed0=9600)
    conv.reset(g.cuda())
    lens = [2 ** 30] * B
    got = {s: [] for s in probes}
    k = 0
    while any(conv.position(s) - lag < want_frames for s in probes):
        raw = [TP.raw_count(s, k, hop) for s in range(B)]
        n = [TP.clamp(v, hop) for v in raw]
        at = [conv.position(s) for s in range(B)]
        assert max(a + c for a, c in zip(at, n)) <= T
        u, z = SC.tick_inputs(unit, noise, at, n, lens, hop, nlag)
        out, got_n = conv.tick(u.cuda(), raw, z.cuda())
        assert got_n == n and out.shape == (B, hop * spf)
        for s in range(B):
            assert bool((out[s, n[s] * spf:] == 0).all()) and bool(torch.isfinite(out[s]).all()), (k, s)
        for s in probes:
            f0 = at[s] - lag
            lo, hi = max(f0, 0), f0 + n[s]
            assert bool((out[s, :max(lo - f0, 0) * spf] == 0).all())
            if hi > lo:
                got[s].append(out[s, (lo - f0) * spf:n[s] * spf].cpu())
        k += 1
        assert k < 200
    assert conv._pos.tolist() == [conv.position(s) for s in range(B)]
    eng = model.engine()
    for s in probes:
        fed = conv.position(s)
        have = torch.cat(got[s])
        assert have.numel() == (fed - lag) * spf >= want_frames * spf
        whole = eng.infer_batch_ragged(unit[s:s + 1, :, :fed].cuda(), g[s:s + 1].cuda(), noise[s:s + 1, :, :fed].cuda(),
                                       torch.tensor([fed], dtype=torch.int32))[0, 0].cpu()
        SC.compare(whole[:have.numel()], have, f"stated size slot {s}: {have.numel() // spf} frames delivered in {k} ticks")


# ---------------------------------------------------------------- status codes
@pytest.mark.parametrize("form", ["ptr", "rng"])
def test_status_codes(lib, dev, form):
    """The refusals on real device buffers: nothing is launched, so state, pos and out stay as they were."""
    import quickvc_official_amd as q
    import config_space as CS
    from quickvc_official_amd import lib as L
    R = GpuRunner(lib, ROW, 5, form)
    for b, n in enumerate(LENS):
        R.reset_slot(b, n)
    unit, _g, noise = SC.row_inputs(ROW)
    u, z = (t.cuda() for t in SC.tick_inputs(unit, noise, [0] * S, [5] * S, LENS, 5, R.nlag))
    cd = torch.full((S,), 5, dtype=torch.int32, device=dev)
    R._out.fill_(7.0)
    torch.cuda.synchronize()
    before = (R.state(), R.positions(), R._out.clone())
    single = L.make_config(q.SynthesizerTrn(641, 32, **q.ISTFT_MODEL_CONFIG).model_config)
    one_up = L.make_config(CS.problem("one_up8")[1])
    fn, draw = (lib.qvc_stream_tick, _ptr(z)) if form == "ptr" else (lib.qvc_stream_tick_rng, ctypes.byref(R.rng))

    def tick(cfgp=R.p, B=S, hop=5, n_new=_ptr(cd), ns=R.n_state, nw=R.n_ws, draw_=draw):
        return fn(cfgp, _ptr(R.blob), _ptr(R._state), ns, _ptr(u), _ptr(R.g), draw_, _ptr(R._out), B, hop, n_new, _ptr(R._pos), _ptr(R._len),
                  _ptr(R._ws), nw, R._stream())
    assert tick(n_new=None) == -1 and tick(hop=0) == -1 and tick(B=0) == -1 and tick(draw_=None) == -1
    assert tick(ns=R.n_state - 1) == -5 and tick(nw=R.n_ws - 1) == -5 and tick(nw=R.n_ws_step) == -5
    for bad in (single, one_up):
        assert tick(cfgp=ctypes.byref(bad)) == -2
        assert lib.qvc_stream_tick_workspace_bytes(ctypes.byref(bad), S, 5) == -2
    torch.cuda.synchronize()
    assert torch.equal(R.state(), before[0]) and R.positions() == before[1] and torch.equal(R._out, before[2])
    assert tick() == 0
    torch.cuda.synchronize()
    assert R.positions() == [5] * S


# ---------------------------------------------------------------- memory contract
@pytest.mark.parametrize("form", ["ptr", "rng"])
def test_memory_contract(lib, dev, form):
    """Every qvc_stream_tick[_rng] of the row's streams at hop 5 under the fixed pattern to the flush, every caller-owned
    buffer in a guarded arena (tests/memguard.py) of exactly the queried size.  state, workspace (stale from tick to
    tick), out, pos_dev and len_dev start from the fill (0x00 / 0x3C / 0xFF = NaN); a fourth run starts from a workspace
    another call has used (a lockstep step of other streams on the same workspace arena).  Guards intact, inputs
    unchanged, outputs bit-equal across the fills and equal to the unguarded run's."""
    unit, _g, noise = SC.row_inputs(ROW)
    hop = 5
    _R, plain, _seen = _cut(ROW, hop, form, "pattern")
    fills = M.FILLS + [(0xFF, 0xFF)]
    for i, (fill, guard) in enumerate(fills):
        A = M.ArenaSet(dev, fill, guard)
        R = GpuRunner(lib, ROW, hop, form, arenas=A)
        if i == len(M.FILLS):        # the stale workspace: a lockstep step of other inputs, on a state that is then re-started
            for b in range(S):
                R.reset_slot(b, 2 ** 30)
            R.step(torch.randn(S, 256, hop), torch.randn(S, noise.shape[1], hop))
        ticks = SC.run_streams(R, unit, noise, LENS, TP.raw_count, junk=NAN if fill == 0xFF else 123.0)
        damaged = A.check()
        assert not damaged, f"fill {fill:#x}: {M.describe_guards(damaged)}"
        assert len(ticks) == len(plain)
        for (a0, n0, o0), (a1, n1, o1) in zip(plain, ticks):
            assert a0 == a1 and n0 == n1
            assert M.bits_equal(o0, o1), f"the output depends on what the buffers held: run {i} (fill {fill:#x}) differs at {a0}"
