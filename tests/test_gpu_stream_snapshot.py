"""The slot snapshots of the segment rings on an MI355X (run with -m gpu): qvc_stream_export_slots / _import_slots through
the raw C ABI, and StreamSnapshot / export_slot / import_slot / move_slot / rebuilt through the converters, in both forms
of the noise.  The scenarios P4 - P8 are those of tests/test_stream_snapshot_host.py (tests/snapshot_common.py); a moved
stream is compared with GPU output of the offline path (qvc_infer_batch_ragged[_rng] on the whole utterance, same g, same
noise or (seed, key)) at >= 90 dB, the project's streaming bar -- the measured figure and whether the two are bit-equal are
printed.  Added here: the trip through host bytes (P9), the Python refusals (P10), one captured graph of an export plus
an import, the memory contract in guarded arenas, and rebuilt() (P11).
"""
import ctypes
import functools

import pytest
import torch

import memguard as M
import snapshot_common as SN
import stream_tick_common as SC
import tick_patterns as TP
from live_common import SEED, _Model, _debug_switches_at_defaults, dev, lib, twin_library  # noqa: F401
from stream_tick_common import LENS, NAN, ROW, ROW_MB

pytestmark = pytest.mark.gpu
S = len(LENS)


@functools.lru_cache(maxsize=None)
def _model(name):
    mc, sd = SC.row_problem(name)
    return _Model(mc, sd, torch.device("cuda:0"))


@functools.lru_cache(maxsize=None)
def _twin():
    return SN.declare_twin(twin_library())       # host arithmetic only: the ring table


def _ptr(t):
    return None if t is None else t.data_ptr()


def _i64(k):
    return k - (1 << 64) if k >> 63 else k


class GpuRunner:
    """snapshot_common's runner surface over the raw C ABI, B slots.  Buffers come from `arenas` (a memguard.ArenaSet:
    exactly the queried sizes between guards, filled with its fill; `tag` keeps the names of two runs apart) or are plain
    tensors filled with 0xFF."""

    def __init__(self, lib, name, B, hop, form, arenas=None, tag=""):
        from quickvc_official_amd import lib as L
        from quickvc_official_amd.engine import aligned_empty
        model = _model(name)
        self.eng, self.lib, self.form, self.B, self.hop, self.A, self.tag = model.engine(), lib, form, B, hop, arenas, tag
        eng, d = self.eng, self.eng.device
        self.p = ctypes.byref(eng.cfg)
        self.n_state, self.n_ws, self.lag, self.nlag = eng.stream_tick_sizes(B, hop)
        self.n_ws_step = eng.stream_sizes(B, hop)[1]
        self.n_snap = eng.stream_snapshot_bytes()
        self.spf = model.samples_per_frame
        gin = SC.row_inputs(name)[1].shape[1]
        if arenas is None:
            self._state, self._ws = aligned_empty(self.n_state, d).fill_(0xFF), aligned_empty(self.n_ws, d).fill_(0xFF)
            self._out = torch.empty(B, hop * self.spf, device=d)
            self._pos, self._len = torch.full((B,), 12345, dtype=torch.int32, device=d), torch.full((B,), -7, dtype=torch.int32, device=d)
            self.g, self._keys = torch.zeros(B, gin, device=d), torch.zeros(B, dtype=torch.int64, device=d)
        else:
            self._state, self._ws = arenas.scratch(tag + "state", self.n_state), arenas.scratch(tag + "workspace", self.n_ws)
            self._out = arenas.output(tag + "out", torch.float32, (B, hop * self.spf))
            self._pos, self._len = arenas.output(tag + "pos_dev", torch.int32, (B,)), arenas.output(tag + "len_dev", torch.int32, (B,))
            self.g = arenas.input(tag + "g", torch.zeros(B, gin), track=False)
            self._keys = arenas.input(tag + "keys_dev", torch.zeros(B, dtype=torch.int64), track=False)
        self.blob = eng.blob
        self.rng = L.QvcNoiseRng(SEED, _ptr(self._keys), 1.0)
        self.table = SC.ring_table(_twin(), eng.cfg, B, hop)

    def _stream(self):
        return torch.cuda.current_stream().cuda_stream

    def reset_slot(self, b, length):
        st = self.lib.qvc_stream_reset_slot(self.p, _ptr(self._state), self.n_state, self.B, self.hop, b, int(length), _ptr(self._pos),
                                            _ptr(self._len), self._stream())
        assert st == 0, st

    def set_row(self, b, g_row, key):
        self.g[b] = g_row.to(self.g.device)
        self._keys[b] = _i64(key)

    def admit(self, b, length, g_row, key):
        self.reset_slot(b, length)
        self.set_row(b, g_row, key)

    def idle(self, b):
        self.reset_slot(b, 0)

    def state(self):
        return self._state.cpu()

    def books(self):
        return self._pos.cpu(), self._len.cpu()

    def positions(self):
        return self._pos.tolist()

    def fill_state(self, byte):
        self._state.fill_(byte)

    def snap_buffer(self, n, name="snap"):
        from quickvc_official_amd.engine import aligned_empty
        if self.A is not None:
            return self.A.scratch(self.tag + name, n * self.n_snap)
        return aligned_empty(n * self.n_snap, self.eng.device).fill_(0xEE)

    def export(self, slots, into=None):
        snap = self.snap_buffer(len(slots)) if into is None else into
        st = self.lib.qvc_stream_export_slots(self.p, _ptr(self._state), self.n_state, self.B, self.hop, SN.slot_array(slots), len(slots),
                                              _ptr(self._pos), _ptr(self._len), _ptr(snap), snap.numel(), self._stream())
        assert st == 0, st
        return snap

    def import_(self, slots, snap):
        st = self.lib.qvc_stream_import_slots(self.p, _ptr(self._state), self.n_state, self.B, self.hop, SN.slot_array(slots), len(slots),
                                              _ptr(self._pos), _ptr(self._len), _ptr(snap), snap.numel(), self._stream())
        assert st == 0, st

    def _call(self, tick, u_new, z_new, raw):
        d = self.eng.device
        u, z = u_new.to(d), z_new.to(d)
        if self.A is not None:
            self._out.view(torch.uint8).fill_(self.A.fill)
        else:
            self._out.fill_(NAN)
        stem = "qvc_stream_tick" if tick else "qvc_stream_step"
        fn, draw = (getattr(self.lib, stem), _ptr(z)) if self.form == "ptr" else (getattr(self.lib, stem + "_rng"), ctypes.byref(self.rng))
        head = (self.p, _ptr(self.blob), _ptr(self._state), self.n_state, _ptr(u), _ptr(self.g), draw, _ptr(self._out), self.B, self.hop)
        if tick:
            cd = torch.tensor(raw, dtype=torch.int32, device=d)
            st = fn(*head, _ptr(cd), _ptr(self._pos), _ptr(self._len), _ptr(self._ws), self.n_ws, self._stream())
        else:
            st = fn(*head, _ptr(self._pos), _ptr(self._len), _ptr(self._ws), self.n_ws_step, self._stream())
        torch.cuda.synchronize()
        assert st == 0, (stem, st)
        return self._out.clone()

    def tick(self, u_new, z_new, raw):
        return self._call(True, u_new, z_new, raw)

    def step(self, u_new, z_new):
        out = self._call(False, u_new, z_new, None)
        self._pos += self.hop
        return out


class ConvRunner:
    """The same surface over a converter (StreamTickConverter, or StreamConverter: steps only)."""

    def __init__(self, conv):
        self.conv, self.B, self.hop, self.lag, self.nlag, self.spf = conv, conv.streams, conv.hop, conv.lag, conv.noise_lag, conv.spf
        conv._state.fill_(0xFF)
        torch.cuda.synchronize()

    def admit(self, b, length, g_row, key):
        self.conv.start(b, g_row.cuda(), length=length, key=key)

    def set_row(self, b, g_row, key):      # an imported stream brought both with it
        pass

    def idle(self, b):
        self.conv.free_slot(b)

    def positions(self):
        got = self.conv._pos.tolist()
        assert got == [self.conv.position(b) for b in range(self.B)], "the device positions and the host mirror disagree"
        return got

    def tick(self, u, z, n):
        return self.conv.tick(u.cuda(), n, None if self.conv._rng is not None else z.cuda())[0]

    def step(self, u, z):
        return self.conv.step(u.cuda(), None if self.conv._rng is not None else z.cuda())


def conv_move(src, b, dst, b2):
    """snapshot_common.move through StreamConverter.move_slot."""
    s, at, log = src.sid[b], src.at[b], src.log[src.sid[b]]
    src.R.conv.move_slot(b, dst.R.conv, b2)
    src.sid[b], src.at[b] = None, 0
    dst.arrive(b2, s, at, log)
    assert not src.R.conv.occupied(b) and dst.R.conv.position(b2) == at


@functools.lru_cache(maxsize=None)
def _whole(name, form):
    """The GPU's whole-utterance conversion of the row's three streams; computed once, read-only."""
    eng = _model(name).engine()
    unit, g, noise = (t.cuda() for t in SC.row_inputs(name))
    frames = torch.tensor(LENS, dtype=torch.int32)
    if form == "ptr":
        return eng.infer_batch_ragged(unit, g, noise, frames).clone().cpu()
    return eng.infer_batch_ragged(unit, g, None, frames, rng=(SEED, SN.KEYS, 1.0)).clone().cpu()


def _make(lib, name, form):
    return lambda B, hop: GpuRunner(lib, name, B, hop, form)


def _make_conv(name, form, cls=None, graph=True):
    from quickvc_official_amd.streaming import StreamTickConverter
    cls = cls or StreamTickConverter
    return lambda B, hop: ConvRunner(cls(_model(name), B, hop, use_graph=graph, seed=SEED if form == "rng" else None))


# ---------------------------------------------------------------- P4 - P8 through the raw C ABI
@pytest.mark.parametrize("name,hop,form", [(ROW, 4, "ptr"), (ROW, 5, "rng"), (ROW_MB, 5, "ptr")])
def test_round_trip_through_a_wiped_state(lib, dev, name, hop, form):
    SN.round_trip(_make(lib, name, form), name, hop)


@pytest.mark.parametrize("name,hop,form", [(ROW, 4, "rng"), (ROW_MB, 5, "ptr")])
def test_another_slot_same_geometry(lib, dev, name, hop, form):
    SN.same_geometry(_make(lib, name, form), name, hop, _whole(name, form))


@pytest.mark.parametrize("name,form", [(ROW, "ptr"), (ROW, "rng"), (ROW_MB, "rng")])
def test_to_one_slot_and_another_hop(lib, dev, name, form):
    SN.to_one_slot(_make(lib, name, form), name, _whole(name, form))


@pytest.mark.parametrize("name,form", [(ROW, "ptr"), (ROW, "rng"), (ROW_MB, "ptr")])
def test_into_a_busy_run_of_another_hop(lib, dev, name, form):
    SN.to_three_slots(_make(lib, name, form), name, _whole(name, form))


@pytest.mark.parametrize("s,calls_before,form", [(0, 0, "ptr"), (2, 3, "rng")])
def test_edges(lib, dev, s, calls_before, form):
    SN.edge(_make(lib, ROW, form), ROW, _whole(ROW, form), s, calls_before)


@pytest.mark.parametrize("name", [ROW, ROW_MB])
def test_exactly_what_is_touched(lib, dev, name):
    SN.touched(_make(lib, name, "ptr"), name)


# ---------------------------------------------------------------- P3 on real buffers
def test_status_codes_leave_everything_alone(lib, dev):
    """Every refusal on real device buffers: nothing is launched, so state, pos, len and snap stay bit for bit."""
    import quickvc_official_amd as q
    import config_space as CS
    from quickvc_official_amd import lib as L
    A = SN.Seats(GpuRunner(lib, ROW, 3, 5, "ptr"), ROW)
    for s in range(3):
        A.admit(s, s)
    A.call()
    R = A.R
    snap = R.snap_buffer(2)
    torch.cuda.synchronize()
    before = (R.state(), *R.books(), snap.cpu())
    single = L.make_config(q.SynthesizerTrn(641, 32, **q.ISTFT_MODEL_CONFIG).model_config)
    one_up = L.make_config(CS.problem("one_up8")[1])
    for fn in (lib.qvc_stream_export_slots, lib.qvc_stream_import_slots):
        def call(cfgp=R.p, state=_ptr(R._state), ns=R.n_state, B=3, hop=5, slots=(0, 2), n=2, pos=_ptr(R._pos), ln=_ptr(R._len), sn=_ptr(snap),
                 nb=snap.numel()):
            return fn(cfgp, state, ns, B, hop, None if slots is None else SN.slot_array(slots), n, pos, ln, sn, nb, R._stream())
        for null in ("cfgp", "state", "pos", "ln", "sn", "slots"):
            assert call(**{null: None}) == -1, null
        assert call(B=0) == -1 and call(n=0) == -1 and call(slots=(0, 3)) == -1 and call(slots=(-1, 0)) == -1
        assert call(hop=0) == -1
        for bad in (single, one_up):
            assert call(cfgp=ctypes.byref(bad)) == -2 and lib.qvc_stream_snapshot_bytes(ctypes.byref(bad)) == -2
        assert call(ns=R.n_state - 1) == -5 and call(nb=snap.numel() - 1) == -5
        assert call(state=_ptr(R._state) + 4) == -1 and call(sn=_ptr(snap) + 64) == -1
        # the order of the checks
        assert call(slots=(0, 3), cfgp=ctypes.byref(single)) == -1 and call(cfgp=ctypes.byref(single), ns=1) == -2
        assert call(ns=1, state=_ptr(R._state) + 4) == -5
    torch.cuda.synchronize()
    after = (R.state(), *R.books(), snap.cpu())
    assert all(torch.equal(x, y) for x, y in zip(before, after)), "a refused call wrote"
    assert call() == 0


# ---------------------------------------------------------------- the converters: P5, P6, P9, P10
@pytest.mark.parametrize("form,cls", [("ptr", "StreamTickConverter"), ("rng", "StreamTickConverter"), ("ptr", "StreamConverter")])
def test_move_slot_inside_one_converter(lib, dev, form, cls):
    """P5 through move_slot(0, self, 2).  StreamConverter has no tick: its run is steps alone."""
    from quickvc_official_amd import streaming
    make = _make_conv(ROW, form, getattr(streaming, cls))
    if cls == "StreamTickConverter":
        return SN.same_geometry(make, ROW, 4, _whole(ROW, form), mover=conv_move)
    A, T = SN.Seats(make(3, 4), ROW), SN.Seats(make(3, 4), ROW)
    for X in (A, T):
        X.admit(0, 0)
        X.admit(1, 1)
    for _ in range(3):
        assert torch.equal(A.call(), T.call())
    conv_move(A, 0, A, 2)
    A.admit(0, 2)
    while not A.all_done():
        oa, ot = A.call(), T.call()
        assert torch.equal(oa[2], ot[0]) and torch.equal(oa[1], ot[1])
    for s in range(3):
        SN.check(_whole(ROW, form), A, s, f"StreamConverter: stream {s} after move_slot")


def test_move_slots_swaps_two_streams_in_one_call(lib, dev):
    """move_slots([0, 1], self, [1, 0]): one export and one import whose source and destination slots overlap.  Each stream
    goes on in the other's slot, torch.equal to the unmoved run call by call."""
    make = _make_conv(ROW, "rng")
    A, T = SN.Seats(make(3, 5), ROW), SN.Seats(make(3, 5), ROW)
    for X in (A, T):
        X.admit(0, 0)
        X.admit(1, 1)
    for k in range(3):
        plan = None if k < 2 else (lambda s: 3 - s)
        assert torch.equal(A.call(plan), T.call(plan))
    conv = A.R.conv
    for bad in (([0, 0], [1, 2]), ([0], [1, 2]), ([0, 1], [2, 2]), ([3], [0])):
        with pytest.raises(ValueError):
            conv.move_slots(bad[0], conv, bad[1])
    conv.move_slots([0, 1], conv, [1, 0])
    A.sid[:2], A.at[:2] = [1, 0], [A.at[1], A.at[0]]
    assert conv.occupied(0) and conv.occupied(1) and not conv.occupied(2)
    k = 0
    while not A.all_done():
        oa, ot = A.call(SN.mixed(k)), T.call(SN.mixed(k))
        assert bool(torch.isfinite(ot).all()) and torch.equal(oa[1], ot[0]) and torch.equal(oa[0], ot[1]), k
        k += 1
    assert k > 5
    for s in (0, 1):
        SN.check(_whole(ROW, "rng"), A, s, f"move_slots swap: stream {s}")


@pytest.mark.parametrize("form", ["ptr", "rng"])
def test_move_slot_between_converters(lib, dev, form):
    """P6 through move_slot between two converters of other batch sizes and hops (their side streams ordered by wait_stream)."""
    SN.to_one_slot(_make_conv(ROW, form), ROW, _whole(ROW, form), mover=conv_move)
    SN.to_three_slots(_make_conv(ROW, form, graph=False), ROW, _whole(ROW, form), mover=conv_move)


@pytest.mark.parametrize("form", ["ptr", "rng"])
def test_through_the_host(lib, dev, form):
    """P9: snap.cpu().tobytes() -> frombytes() -> .to(device) -> import_slot gives P4's equality."""
    from quickvc_official_amd.streaming import StreamSnapshot
    make = _make_conv(ROW, form)
    A, T = SN.Seats(make(3, 5), ROW), SN.Seats(make(3, 5), ROW)
    for X in (A, T):
        X.admit(0, 0)
        X.admit(1, 1)
    for k in range(3):
        plan = None if k < 2 else (lambda s: 3 - s)
        assert torch.equal(A.call(plan), T.call(plan))
    conv = A.R.conv
    raws = [conv.export_slot(b).cpu().tobytes() for b in (0, 1)]
    conv._state.fill_(0xFF)
    conv._g[:2].fill_(NAN)
    for b, raw in enumerate(raws):
        snap = StreamSnapshot.frombytes(raw)
        assert snap.data.device.type == "cpu" and snap.position == A.at[b] and snap.length == LENS[b] and snap.key == SN.KEYS[b]
        assert snap.rng == ((SEED, 1.0) if form == "rng" else None) and snap.tag == conv.snapshot_tag()
        conv.import_slot(b, snap.to(dev))
    k = 0
    while not A.all_done():
        oa, ot = A.call(SN.mixed(k)), T.call(SN.mixed(k))
        assert bool(torch.isfinite(ot).all()) and torch.equal(oa, ot), k
        k += 1
    # a host snapshot is staged by import_slot itself
    conv.import_slot(2, StreamSnapshot.frombytes(raws[0]))
    assert conv.position(2) == StreamSnapshot.frombytes(raws[0]).position


def test_python_refusals(lib, dev):
    """P10: another model's snapshot, or a generator-form snapshot under another seed, raises before anything is written;
    the windowed converters have no snapshots."""
    from quickvc_official_amd.streaming import LiveConverter, StreamTickConverter, TickConverter
    a = StreamTickConverter(_model(ROW), 3, 4, use_graph=False, seed=SEED)
    other = StreamTickConverter(_model(ROW_MB), 1, 4, use_graph=False, seed=SEED)
    reseeded = StreamTickConverter(_model(ROW), 1, 5, use_graph=False, seed=SEED + 1)
    unseeded = StreamTickConverter(_model(ROW), 1, 5, use_graph=False)
    g = SC.row_inputs(ROW)[1].cuda()
    a.start(0, g[0], length=37, key=7)
    snap = a.export_slot(0)
    assert snap.rng == (SEED, 1.0) and snap.tag != other.snapshot_tag()
    for dst in (other, reseeded, unseeded):
        dst._state.fill_(0x5A)
        torch.cuda.synchronize()
        before = (dst._state.cpu(), dst._pos.cpu(), dst._len.cpu(), dst._g.cpu(), dst._keys.cpu(), dst.position(0))
        with pytest.raises(ValueError):
            dst.import_slot(0, snap)
        with pytest.raises(ValueError):
            a.move_slot(0, dst, 0)
        torch.cuda.synchronize()
        after = (dst._state.cpu(), dst._pos.cpu(), dst._len.cpu(), dst._g.cpu(), dst._keys.cpu(), dst.position(0))
        assert all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(before, after))
    assert a.occupied(0) and a.position(0) == 0
    with pytest.raises(ValueError):
        a.export_slot(3)
    for cls in (LiveConverter, TickConverter):
        live = cls(_model(ROW), 1, 4, 2, use_graph=False)
        for refused in (lambda: live.export_slot(0), lambda: live.import_slot(0, snap), lambda: live.move_slot(0, live, 0), lambda: live.rebuilt(2)):
            with pytest.raises(ValueError, match="C \\+ L input frames"):
                refused()


# ---------------------------------------------------------------- P11
@pytest.mark.parametrize("form", ["ptr", "rng"])
def test_one_graph_of_export_and_import(lib, dev, form):
    """Export of slot 0 plus import into slot 2, captured once and replayed at two stream positions: after each replay slot
    2, fed what slot 0 is fed, is torch.equal to it call by call (between the replays slot 2 falls behind on purpose)."""
    A = SN.Seats(GpuRunner(lib, ROW, 3, 4, form), ROW)
    A.admit(0, 0)
    A.admit(1, 1)
    R = A.R
    snap = R.snap_buffer(1)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        R.export([0], into=snap)                 # warm-up (code objects); slot 2 is idle again behind it
        R.import_([2], snap)
        R.idle(2)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            R.export([0], into=snap)
            R.import_([2], snap)
    torch.cuda.synchronize()
    A.call()
    A.call(lambda s: 3)
    for replay, calls in ((0, 3), (1, 100)):
        graph.replay()
        torch.cuda.synchronize()
        A.arrive(2, 0, A.at[0], [])
        k = 0
        while k < calls and not A.all_done():
            out = A.call(SN.mixed(k + replay))
            assert bool(torch.isfinite(out).all()) and torch.equal(out[2], out[0]), (replay, k)
            k += 1
        assert k == calls or replay == 1
        if replay == 0:                          # slot 2 stays behind for a tick
            A.sid[2] = None
            A.call(lambda s: 2)
    assert A.all_done()


@pytest.mark.parametrize("form", ["ptr", "rng"])
def test_memory_contract(lib, dev, form):
    """state, snap (exactly n_slots * snapshot_bytes), pos and len between guards, under the fills 0x00 / 0x3C / 0xFF: two
    slots of a 3-slot hop-4 run exported in one call and imported into a 3-slot hop-5 run whose third slot carries another
    stream.  Guards intact, every output bit-identical across the fills."""
    runs = []
    for fill, guard in M.FILLS:
        arenas = M.ArenaSet(dev, fill, guard)
        A = SN.Seats(GpuRunner(lib, ROW, 3, 4, form, arenas=arenas, tag="a."), ROW)
        B = SN.Seats(GpuRunner(lib, ROW, 3, 5, form, arenas=arenas, tag="b."), ROW)
        A.admit(0, 0)
        A.admit(1, 1)
        B.admit(1, 2)
        outs = [A.call(), A.call(lambda s: 3), B.call()]
        snap = A.R.export([0, 1])
        assert snap.numel() == 2 * A.R.n_snap
        B.R.import_([2, 0], snap)
        B.arrive(2, 0, A.at[0], A.log[0])
        B.arrive(0, 1, A.at[1], A.log[1])
        k = 0
        while not B.all_done():
            outs.append(B.call(SN.mixed(k)))
            k += 1
        damaged = arenas.check()
        assert not damaged, f"fill {fill:#x}: {M.describe_guards(damaged)}"
        runs.append(outs)
        if fill == 0xFF:
            for s in range(3):
                SN.check(_whole(ROW, form), B, s, f"guarded arenas, fill 0xFF, {form}: stream {s}")
    for other in runs[1:]:
        assert len(other) == len(runs[0])
        for k, (x, y) in enumerate(zip(runs[0], other)):
            assert M.bits_equal(x, y), f"the output depends on what the buffers held: call {k}"


@pytest.mark.parametrize("form", ["ptr", "rng"])
def test_rebuilt_grows_and_changes_the_hop(lib, dev, form):
    """rebuilt(streams=1 -> 3) and rebuilt(hop_frames=4 -> 5) on a StreamTickConverter, the second with three streams in
    flight: every stream's concatenated output meets the bar."""
    from quickvc_official_amd.streaming import StreamTickConverter
    A = SN.Seats(_make_conv(ROW, form)(1, 4), ROW)
    A.admit(0, 0)
    A.call()
    A.call()
    A.call(lambda s: 3)
    assert A.at == [11]
    with pytest.raises(ValueError):
        A.R.conv.rebuilt(streams=0)
    grown = A.R.conv.rebuilt(streams=3)
    assert type(grown) is StreamTickConverter and (grown.streams, grown.hop) == (3, 4) and grown._rng == A.R.conv._rng
    assert grown.position(0) == 11 and grown.occupied(0) and (grown._graph is not None or grown._rng_graph is not None)
    B = SN.Seats.__new__(SN.Seats)
    B.__dict__.update(A.__dict__)
    B.R, B.sid, B.at = ConvRunner.__new__(ConvRunner), [0, None, None], [11, 0, 0]
    B.R.__dict__.update(conv=grown, B=3, hop=4, lag=grown.lag, nlag=grown.noise_lag, spf=grown.spf)
    B.admit(1, 1)
    B.admit(2, 2)
    B.call()
    B.call(SN.pattern(1))
    with pytest.raises(ValueError):
        grown.rebuilt(streams=2)
    wider = grown.rebuilt(hop_frames=5)
    assert (wider.streams, wider.hop) == (3, 5) and [wider.position(b) for b in range(3)] == B.at
    B.R.__dict__.update(conv=wider, hop=5)
    B.finish(SN.mixed)
    for s in range(3):
        SN.check(_whole(ROW, form), B, s, f"rebuilt 1 -> 3 slots, hop 4 -> 5, {form}: stream {s}")
