"""What the two test files of the segment rings' tick form share (tests/test_stream_tick_host.py on the CPU twin,
tests/test_gpu_stream_tick.py on the GPU): the shapes the issue names, a runner per side with ONE surface -- reset_slot /
tick / step / state / positions --, the loop that feeds a set of streams tick by tick, and the checks of a tick's rows.

The loop checks at EVERY tick what the contract says of every slot: pos advanced by the clamped count; for an idle slot
(n = 0) the bytes of its rows of every ring (slot_range over the ring table) and its pos bit-equal before and after, and a
row of zeros in `out`; samples behind the n delivered frames exactly 0.0.
"""
import ctypes
import functools

import torch

import config_space as CS
import tick_patterns as TP
from helpers import snr_db

NAN = float("nan")
WN = (2, 1, 2)                     # (enc_layers, flow_layers, n_flows) at kernel 5: a lag of a few tens of frames
LENS = [37, 23, 9]                 # the end falls inside a tick; 9 ends inside the first tile of every stage
HOPS = (4, 5)
ROW, ROW_MB = "up16_k17_up2_k2", "mb_up16_up1"
BAR_DB = 90.0


@functools.lru_cache(maxsize=None)
def row_problem(name, wn=WN):
    """(model_config, state dict) of a row of the configuration space with the short WaveNet, as live_common._row_model."""
    cfg, mc, sd = CS.problem(name)
    keys = dict(wn_kernel_size=5, enc_layers=wn[0], flow_layers=wn[1], n_flows=wn[2])
    cfg, mc = dict(cfg, **keys), dict(mc, **keys)
    return mc, CS.wn_state_dict(dict(sd), cfg)


@functools.lru_cache(maxsize=None)
def row_inputs(name, seed0=9700):
    """(unit, g, noise) on the host for three streams of max(LENS) frames; read-only."""
    from quickvc_official_amd.synth import make_synthetic_inputs
    mc, _sd = row_problem(name)
    unit, g, noise = make_synthetic_inputs(len(LENS), max(LENS), 256, mc["inter_channels"], mc["gin_channels"], seed0=seed0)
    return unit.float().contiguous(), g.float().contiguous(), noise.float().contiguous()


def declare_twin(lib):
    """The stream-tick exports of tools/emu_twin.cpp."""
    from quickvc_official_amd import lib as L
    P, I, Lg, V = ctypes.POINTER, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    lib.qvc_emu_stream_tick.restype = ctypes.c_int
    lib.qvc_emu_stream_tick.argtypes = [P(L.QvcConfig), V, V, Lg, V, V, V, V, I, I, V, V, V, V, Lg]
    lib.qvc_emu_twin_stream_step.restype = ctypes.c_int
    lib.qvc_emu_twin_stream_step.argtypes = [P(L.QvcConfig), V, V, Lg, V, V, V, V, I, I, V, V, V, Lg]
    lib.qvc_emu_stream_reset_slot.restype = ctypes.c_int
    lib.qvc_emu_stream_reset_slot.argtypes = [P(L.QvcConfig), V, Lg, I, I, I, I, V, V]
    lib.qvc_emu_stream_ring.restype = ctypes.c_int
    lib.qvc_emu_stream_ring.argtypes = [P(L.QvcConfig), I, I, I, I, P(Lg)]
    lib.qvc_emu_stream_tick_frozen.restype = ctypes.c_int
    lib.qvc_emu_stream_tick_frozen.argtypes = [P(L.QvcConfig), I, I]
    lib.qvc_emu_stream_tick_counts.restype = None
    lib.qvc_emu_stream_tick_counts.argtypes = [P(Lg)]
    lib.qvc_emu_twin_counts.restype = None
    lib.qvc_emu_twin_counts.argtypes = [P(Lg)]
    return lib


def ring_table(twin, cfg, B, hop):
    """[slot][ring] -> (offset, bytes, rows, keep, hopb): the slot's range of every ring of the segment rings' table."""
    table = []
    for b in range(B):
        per, i = [], 0
        while True:
            v = (ctypes.c_int64 * 5)()
            st = twin.qvc_emu_stream_ring(ctypes.byref(cfg), B, hop, b, i, v)
            if st != 0:
                assert st == -1 and i > 0
                break
            per.append(tuple(int(x) for x in v))
            i += 1
        table.append(per)
    return table


def kept_bytes(state, table, b):
    """The bytes of slot b a later call can still read: the kept part of every row of every ring, concatenated."""
    parts = []
    for off, n, rows, keep, hopb in table[b]:
        parts.append(state[off:off + n].reshape(rows, keep + hopb)[:, :keep].reshape(-1))
    return torch.cat(parts)


def slot_bytes(state, table, b):
    return torch.cat([state[off:off + n] for off, n, _r, _k, _h in table[b]])


def _aligned(n, fill):
    raw = torch.full((n + 256,), fill, dtype=torch.uint8)
    shift = (-raw.data_ptr()) % 256
    return raw, raw[shift:shift + n]


class TwinRunner:
    """The CPU twin (pointer form of the noise only).  State and workspace start from 0xFF bytes."""
    form = "ptr"

    def __init__(self, built, twin, mc, sd, g, B, hop, dtype="f16", ws_fill=0xFF):
        from quickvc_official_amd import lib as L
        self.built, self.twin, self.B, self.hop = built, twin, B, hop
        self.cfg = L.make_config(dict(mc, operand_dtype=dtype))
        self.p = ctypes.byref(self.cfg)
        self.blob = L.pack_weights(built, self.cfg, sd)
        self.n_state = int(built.qvc_stream_state_bytes(self.p, B, hop))
        self.n_ws = int(built.qvc_stream_tick_workspace_bytes(self.p, B, hop))
        assert self.n_state > 0 and self.n_ws > int(built.qvc_stream_workspace_bytes(self.p, B, hop)) > 0
        self.lag, self.nlag = int(built.qvc_stream_lag_frames(self.p)), int(built.qvc_stream_noise_lag_frames(self.p))
        self.spf = int(self.cfg.hop) * int(self.cfg.subbands) * int(self.cfg.upsample_rates[0]) * int(self.cfg.upsample_rates[1])
        self._k1, self._state = _aligned(self.n_state, 0xFF)
        self._k2, self._ws = _aligned(self.n_ws, ws_fill)
        self._pos = torch.full((B,), 12345, dtype=torch.int32)
        self._len = torch.full((B,), -7, dtype=torch.int32)
        self.g = g.float().contiguous()
        self.table = ring_table(twin, self.cfg, B, hop)

    def reset_slot(self, b, length):
        st = self.twin.qvc_emu_stream_reset_slot(self.p, self._state.data_ptr(), self.n_state, self.B, self.hop, b, int(length),
                                                 self._pos.data_ptr(), self._len.data_ptr())
        assert st == 0, st

    def state(self):
        return self._state.clone()

    def positions(self):
        return self._pos.tolist()

    def tick(self, u_new, z_new, raw):
        counts = torch.tensor(raw, dtype=torch.int32)
        out = torch.full((self.B, self.hop * self.spf), NAN)
        u_new, z_new = u_new.contiguous(), z_new.contiguous()
        st = self.twin.qvc_emu_stream_tick(self.p, self.blob.data_ptr(), self._state.data_ptr(), self.n_state, u_new.data_ptr(), self.g.data_ptr(),
                                           z_new.data_ptr(), out.data_ptr(), self.B, self.hop, counts.data_ptr(), self._pos.data_ptr(),
                                           self._len.data_ptr(), self._ws.data_ptr(), self.n_ws)
        assert st == 0, st
        assert counts.tolist() == list(raw), "n_new was written"
        return out

    def step(self, u_new, z_new):
        """qvc_stream_step on the SAME state and workspace (the step's workspace is a prefix of the tick's)."""
        out = torch.full((self.B, self.hop * self.spf), NAN)
        u_new, z_new = u_new.contiguous(), z_new.contiguous()
        n_ws = int(self.built.qvc_stream_workspace_bytes(self.p, self.B, self.hop))
        st = self.twin.qvc_emu_twin_stream_step(self.p, self.blob.data_ptr(), self._state.data_ptr(), self.n_state, u_new.data_ptr(),
                                                self.g.data_ptr(), z_new.data_ptr(), out.data_ptr(), self.B, self.hop, self._pos.data_ptr(),
                                                self._len.data_ptr(), self._ws.data_ptr(), n_ws)
        assert st == 0, st
        self._pos += self.hop
        return out


def tick_inputs(unit, noise, at, n, lens, hop, nlag, junk=NAN):
    """unit_new / noise_new of one tick on the host: `junk` everywhere but columns [0, n[b]) -- unit frames [at, at + n), noise
    frames [at - nlag, at - nlag + n) -- and there too for frames outside [0, len)."""
    B = len(at)
    u = torch.full((B, unit.shape[1], hop), junk)
    z = torch.full((B, noise.shape[1], hop), junk)
    for b in range(B):
        hi = min(at[b] + n[b], lens[b])
        if hi > at[b]:
            u[b, :, :hi - at[b]] = unit[b, :, at[b]:hi]
        f0 = at[b] - nlag
        lo, hi = max(f0, 0), min(f0 + n[b], lens[b])
        if hi > lo:
            z[b, :, lo - f0:hi - f0] = noise[b, :, lo:hi]
    return u, z


def run_streams(R, unit, noise, lens, count_of, junk=NAN, watch=None, call=None, between=None, max_ticks=400):
    """Starts stream b in slot b (reset_slot) and ticks with n_new[b] = count_of(b, tick, hop) (raw: the library clamps)
    until the slots in `watch` (default: all) have flushed.  call(k) -> "tick" | "step" chooses the entry point of call k
    (a step needs every count == hop); between(k, R, at) runs in front of call k and may reset slots (it returns the new
    positions).  -> [(positions before, clamped counts, out (B, hop * spf) on the host)]"""
    B, hop = R.B, R.hop
    watch = list(range(B)) if watch is None else watch
    for b in range(B):
        R.reset_slot(b, lens[b])
    assert R.positions() == [0] * B
    at, ticks, k = [0] * B, [], 0
    while any(at[b] - R.lag < lens[b] for b in watch):
        if between is not None:
            at = between(k, R, at)
        raw = [count_of(b, k, hop) for b in range(B)]
        n = [TP.clamp(v, hop) for v in raw]
        u, z = tick_inputs(unit, noise, at, n, lens, hop, R.nlag, junk)
        before = R.state() if 0 in n else None
        if call is not None and call(k) == "step":
            assert n == [hop] * B
            out = R.step(u, z)
        else:
            out = R.tick(u, z, raw)
        out = out.cpu()
        now = [a + c for a, c in zip(at, n)]
        assert R.positions() == now, (k, R.positions(), now)
        after = R.state() if 0 in n else None
        for b in range(B):
            assert bool((out[b, n[b] * R.spf:] == 0).all()), (k, b, "not zero behind the delivered frames")
            if n[b] == 0:
                assert torch.equal(slot_bytes(after, R.table, b), slot_bytes(before, R.table, b)), (k, b, "an idle slot's rings changed")
        ticks.append((list(at), n, out))
        at = now
        k += 1
        assert k < max_ticks
    return ticks


def collect(ticks, b, length, lag, spf, what=""):
    """Stream b's delivered samples concatenated (length * spf); exact zeros where a delivered frame lies outside
    [0, length); every frame of the stream delivered exactly once and finite."""
    got = torch.full((length * spf,), NAN)
    for at, n, out in ticks:
        f0 = at[b] - lag
        lo, hi = max(f0, 0), min(f0 + n[b], length)
        head = out[b, :n[b] * spf]
        inside = torch.zeros(n[b] * spf, dtype=torch.bool)
        if hi > lo:
            inside[(lo - f0) * spf:(hi - f0) * spf] = True
            assert bool(torch.isnan(got[lo * spf:hi * spf]).all()), (what, b, at, "a frame delivered twice")
            got[lo * spf:hi * spf] = head[inside]
        assert bool((head[~inside] == 0).all()), (what, b, at, "not zero outside the stream")
    assert bool(torch.isfinite(got).all()), (what, b, "frames never delivered, or not finite")
    return got


def check_pattern_holds(ticks, lens, hop, seen_raw):
    """What the fixed pattern must have exercised: the clamp's two sides, ticks of 0..3 and hop frames, an end inside a
    tick and flush ticks behind it."""
    assert {-3, 0, 1, 2, 3, hop, hop + 5} <= seen_raw
    assert any(at[b] < end < at[b] + n[b] for at, n, _o in ticks for b, end in enumerate(lens)), "no stream ends inside a tick"
    for b, end in enumerate(lens):
        assert any(at[b] >= end and n[b] > 0 for at, n, _o in ticks), b


def compare(want, got, what):
    db = snr_db(want, got)
    print(f"{what}: {db:.1f} dB, bit-equal: {torch.equal(want, got)}")
    assert db >= BAR_DB, (what, db)
    return db
