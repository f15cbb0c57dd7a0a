"""What the two test files of the slot snapshots share (tests/test_stream_snapshot_host.py on the CPU twin,
tests/test_gpu_stream_snapshot.py on the GPU): the snapshot surface a runner adds to stream_tick_common's -- export /
import_ / fill_state / admit / idle --, Seats, the book of which stream sits in which slot of a run, and the scenarios
P4 - P8 of the issue, written once over that surface.

A runner's slots carry streams of the row's three (stream_tick_common.row_inputs, LENS = 37 / 23 / 9 frames); a stream
keeps its g row and its generator key wherever it sits.  Every call is logged per STREAM, so a stream that moved between
runs is collected (stream_tick_common.collect: every frame exactly once, zeros outside the stream) from the ticks of both.
"""
import ctypes

import torch

import stream_tick_common as SC
import tick_patterns as TP
from live_common import _keys
from stream_tick_common import LENS

KEYS = _keys(len(LENS))


def declare_twin(lib):
    """stream_tick_common's exports of tools/emu_twin.cpp and the two of the snapshots."""
    from quickvc_official_amd import lib as L
    SC.declare_twin(lib)
    P, I, Lg, V = ctypes.POINTER, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    for fn in (lib.qvc_emu_stream_export_slots, lib.qvc_emu_stream_import_slots):
        fn.restype = ctypes.c_int
        fn.argtypes = [P(L.QvcConfig), V, Lg, I, I, P(I), I, V, V, V, Lg]
    return lib


def slot_array(slots):
    return (ctypes.c_int32 * len(slots))(*slots)


def layout_bytes(per_slot):
    """The stated size of one snapshot from a slot's ring table: every ring's rows * keep and then 8 bytes for pos and
    len, each carved at the next multiple of 256."""
    off = 0
    for _o, _n, rows, keep, _h in per_slot:
        off = -(-(off + rows * keep) // 256) * 256
    return -(-(off + 8) // 256) * 256


def kept_mask(n_state, table, slots):
    """bool (n_state,): the bytes an import into `slots` may write -- [off, off + keep) of each of their rows of every ring."""
    mask = torch.zeros(n_state, dtype=torch.bool)
    for b in slots:
        for off, n, rows, keep, hopb in table[b]:
            mask[off:off + n].reshape(rows, keep + hopb)[:, :keep] = True
    return mask


class TwinSnapRunner(SC.TwinRunner):
    """stream_tick_common.TwinRunner with the snapshot surface, on the CPU twin (pointer form of the noise)."""

    def __init__(self, built, twin, mc, sd, g, B, hop, **kw):
        super().__init__(built, twin, mc, sd, g[:1].expand(B, -1), B, hop, **kw)
        self.g = self.g.clone()
        self.n_snap = int(built.qvc_stream_snapshot_bytes(self.p))
        assert self.n_snap > 0

    def set_row(self, b, g_row, _key):
        self.g[b] = g_row

    def admit(self, b, length, g_row, key):
        self.reset_slot(b, length)
        self.set_row(b, g_row, key)

    def idle(self, b):
        self.reset_slot(b, 0)

    def export(self, slots):
        _raw, snap = SC._aligned(len(slots) * self.n_snap, 0xEE)
        st = self.twin.qvc_emu_stream_export_slots(self.p, self._state.data_ptr(), self.n_state, self.B, self.hop, slot_array(slots), len(slots),
                                                   self._pos.data_ptr(), self._len.data_ptr(), snap.data_ptr(), snap.numel())
        assert st == 0, st
        return snap

    def import_(self, slots, snap):
        st = self.twin.qvc_emu_stream_import_slots(self.p, self._state.data_ptr(), self.n_state, self.B, self.hop, slot_array(slots), len(slots),
                                                   self._pos.data_ptr(), self._len.data_ptr(), snap.data_ptr(), snap.numel())
        assert st == 0, st

    def fill_state(self, byte):
        self._state.fill_(byte)

    def books(self):
        return self._pos.clone(), self._len.clone()


class Seats:
    """A run and who sits where: slot b carries stream sid[b] of the row's three, or nobody (an idle slot: zeroed rows,
    position 0, length 0).  A runner has stream_tick_common's surface plus admit / idle / export / import_."""

    def __init__(self, R, name):
        self.R, self.name = R, name
        self.unit, self.g, self.noise = SC.row_inputs(name)
        self.sid, self.at, self.log, self.calls = [None] * R.B, [0] * R.B, {}, 0
        for b in range(R.B):
            R.idle(b)

    def admit(self, b, s):
        """A new stream s in slot b."""
        self.R.admit(b, LENS[s], self.g[s], KEYS[s])
        self.sid[b], self.at[b] = s, 0
        self.log.setdefault(s, [])

    def arrive(self, b, s, at, log=None):
        """Stream s, imported into slot b at position `at` (its g row and key follow it); log: its ticks so far."""
        self.R.set_row(b, self.g[s], KEYS[s])
        self.sid[b], self.at[b] = s, at
        self.log[s] = log if log is not None else self.log.get(s, [])

    def leave(self, b, idle=True):
        if idle:
            self.R.idle(b)
            self.at[b] = 0
        self.sid[b] = None

    def call(self, count_of=None, record=True):
        """One call: count_of None = a step (every slot moves by hop, the idle ones too), else a tick in which the slot of
        stream s brings count_of(s) frames (raw; clamped here as the library clamps) and an idle slot nothing."""
        R = self.R
        hop, B = R.hop, R.B
        step = count_of is None
        n = [hop if step else (TP.clamp(count_of(s), hop) if s is not None else 0) for s in self.sid]
        idx = [s if s is not None else 0 for s in self.sid]
        lens = [LENS[s] if s is not None else 0 for s in self.sid]
        u, z = SC.tick_inputs(self.unit[idx], self.noise[idx], self.at, n, lens, hop, R.nlag)
        out = (R.step(u, z) if step else R.tick(u, z, n)).cpu()
        for b, s in enumerate(self.sid):
            if s is not None and record:
                self.log[s].append(([self.at[b]], [n[b]], out[b:b + 1].clone()))
        self.at = [a + c for a, c in zip(self.at, n)]
        assert R.positions() == self.at, (R.positions(), self.at)
        self.calls += 1
        return out

    def done(self, s):
        return self.at[self.sid.index(s)] - self.R.lag >= LENS[s]

    def all_done(self):
        return all(self.done(s) for s in self.sid if s is not None)

    def finish(self, plan, limit=200):
        """plan(k) -> count_of or None, for call k from now on, until every seated stream has flushed."""
        k = 0
        while not self.all_done():
            self.call(plan(k))
            k += 1
            assert k < limit
        return k

    def collect(self, s):
        return SC.collect(self.log[s], 0, LENS[s], self.R.lag, self.R.spf, f"{self.name} stream {s}")


def mixed(k):
    """Call k of a mixed run: steps and pattern ticks alternate."""
    return None if k % 2 == 0 else (lambda s: TP.raw_count(s, k, 64))


def pattern(k):
    return lambda s: TP.raw_count(s, k, 64)


def move(src, b, dst, b2, free=True):
    """Raw-surface move of the stream in slot b of run `src` into slot b2 of run `dst` (Seats): export, import, and the
    source slot left idle."""
    s, at = src.sid[b], src.at[b]
    snap = src.R.export([b])
    dst.R.import_([b2], snap)
    log = src.log[s]
    if free:
        src.leave(b)
    dst.arrive(b2, s, at, log)


def check(whole, seats, s, what):
    n = LENS[s] * seats.R.spf
    return SC.compare(whole[s, 0, :n], seats.collect(s), what)


# ---------------------------------------------------------------- P4
def round_trip(make, name, hop, through=lambda snap: snap):
    """P4: A and T fed identically; after 3 calls A's slots 0 and 1 are exported (one call, two slots), A's whole state
    is filled with 0xFF and the two slots are imported again.  Every later output of A is torch.equal to T's -- nothing
    outside the kept parts is ever read."""
    A, T = Seats(make(3, hop), name), Seats(make(3, hop), name)
    for X in (A, T):
        X.admit(0, 0)
        X.admit(1, 1)
    for k in range(3):
        plan = None if k < 2 else (lambda s: 3 - s)
        oa, ot = A.call(plan), T.call(plan)
        assert torch.equal(oa, ot), k
    snap = A.R.export([0, 1])
    A.R.fill_state(0xFF)
    A.R.import_([0, 1], through(snap))
    k = 0
    while not A.all_done():
        oa, ot = A.call(mixed(k)), T.call(mixed(k))
        assert bool(torch.isfinite(ot).all()) and torch.equal(oa, ot), (k, "the re-imported run differs")
        k += 1
    assert k > 5
    return A, T


# ---------------------------------------------------------------- P5
def same_geometry(make, name, hop, whole, mover=move):
    """P5: after 3 calls A moves slot 0 into its own slot 2; from then on A's row 2 is torch.equal to T's row 0 and A's
    row 1 to T's row 1 at every call.  The freed slot 0 takes the 9-frame stream, which meets the bar against its
    whole-utterance conversion."""
    A, T = Seats(make(3, hop), name), Seats(make(3, hop), name)
    for X in (A, T):
        X.admit(0, 0)
        X.admit(1, 1)
    for k in range(3):
        plan = None if k < 2 else (lambda s: 3 - s)
        assert torch.equal(A.call(plan), T.call(plan)), k
    mover(A, 0, A, 2)
    A.admit(0, 2)
    k = 0
    while not A.all_done():
        oa, ot = A.call(mixed(k)), T.call(mixed(k))
        assert bool(torch.isfinite(oa).all()) and torch.equal(oa[2], ot[0]) and torch.equal(oa[1], ot[1]), (k, "the moved stream differs")
        k += 1
    assert k > 5
    for s in (0, 1, 2):
        check(whole, A, s, f"{name} hop {hop}: stream {s} after the move inside one run")


# ---------------------------------------------------------------- P6
def to_one_slot(make, name, whole, mover=move):
    """P6: two steps and a tick of 3 in a 3-slot hop-4 run (pos 11), then slot 0 continues in a 1-slot hop-5 run: steps, a
    short last tick, the flush."""
    A, B = Seats(make(3, 4), name), Seats(make(1, 5), name)
    for s in range(3):
        A.admit(s, s)
    A.call()
    A.call()
    A.call(lambda s: 3)
    assert A.at == [11, 11, 11]
    mover(A, 0, B, 0)
    while B.at[0] + 5 <= LENS[0]:
        B.call()
    short = LENS[0] - B.at[0]
    assert 0 < short < 5
    B.call(lambda s: short)
    B.finish(lambda k: None)
    check(whole, B, 0, f"{name}: 3 slots hop 4 -> 1 slot hop 5 at pos 11")
    A.finish(mixed)
    for s in (1, 2):
        check(whole, A, s, f"{name}: stream {s} of the run the stream left")


def to_three_slots(make, name, whole, mover=move):
    """P6, the reverse: 1 slot hop 5 (two steps and a tick of 3: pos 13) -> slot 1 of a 3-slot hop-4 run whose slots 0
    and 2 carry other streams, mid-stream."""
    C, D = Seats(make(1, 5), name), Seats(make(3, 4), name)
    C.admit(0, 0)
    C.call()
    C.call()
    C.call(lambda s: 3)
    assert C.at == [13]
    D.admit(0, 1)
    D.admit(2, 2)
    D.call()
    D.call(lambda s: 2)
    mover(C, 0, D, 1)
    D.finish(mixed)
    for s in (0, 1, 2):
        check(whole, D, s, f"{name}: stream {s} of the 3-slot hop-4 run (stream 0 arrived from 1 slot hop 5 at pos 13)")


# ---------------------------------------------------------------- P7
def edge(make, name, whole, s, calls_before, mover=move):
    """P7: stream s moves from a 3-slot hop-4 run into a 1-slot hop-5 run after `calls_before` steps -- 0: a slot that never
    stepped (pos 0, zeroed rows); 3 with the 9-frame stream: one that has ended and is flushing (len < pos).  It meets
    the bar, and it has flushed after as many calls as the unmoved run: the same counts as ticks of one hop-5 run."""
    A, B, U = Seats(make(3, 4), name), Seats(make(1, 5), name), Seats(make(1, 5), name)
    A.admit(1, s)
    U.admit(0, s)
    for _ in range(calls_before):
        A.call()
        U.call(lambda s_: 4)
    if calls_before:
        assert A.at[1] > LENS[s], "the stream has not ended yet"
    mover(A, 1, B, 0)
    assert B.at == U.at
    while not U.all_done():
        assert not B.all_done()
        U.call()
        B.call()
    assert B.all_done() and B.calls + calls_before == U.calls
    check(whole, B, s, f"{name}: stream {s} moved after {calls_before} calls")
    SC.compare(U.collect(s), B.collect(s), f"{name}: stream {s} moved after {calls_before} calls against the unmoved run")


# ---------------------------------------------------------------- P8
def touched(make, name):
    """P8: the bytes of state, pos and len before and after: an export changes nothing; an import changes only the kept
    part of the named slots' rows of every ring, pos[slot] and len[slot] -- and those hold the source's."""
    A, B = Seats(make(3, 4), name), Seats(make(3, 5), name)
    for X in (A, B):
        for s in range(3):
            X.admit(s, s)
    A.call()
    A.call(pattern(4))
    B.call(pattern(5))
    a_state, (a_pos, a_len) = A.R.state(), A.R.books()
    snap = A.R.export([0, 2])
    assert torch.equal(A.R.state(), a_state) and all(torch.equal(x, y) for x, y in zip(A.R.books(), (a_pos, a_len))), "an export wrote"
    b_state, (b_pos, b_len) = B.R.state(), B.R.books()
    keep = snap.clone()
    B.R.import_([2, 1], snap)
    assert torch.equal(snap.cpu(), keep.cpu()), "an import wrote the snapshots"
    after, (pos, ln) = B.R.state(), B.R.books()
    mask = kept_mask(after.numel(), B.R.table, [2, 1])
    assert torch.equal(after[~mask], b_state[~mask]), "an import wrote outside the kept parts of the named slots"
    for src, dst in ((0, 2), (2, 1)):
        assert torch.equal(SC.kept_bytes(after, B.R.table, dst), SC.kept_bytes(a_state, A.R.table, src)), (src, dst)
        assert int(pos[dst]) == int(a_pos[src]) and int(ln[dst]) == int(a_len[src])
    assert int(pos[0]) == int(b_pos[0]) and int(ln[0]) == int(b_len[0])
    assert not torch.equal(after[mask], b_state[mask])
