"""CPU tests (no GPU) of the slot snapshots of the segment rings (include/qvc.h: qvc_stream_snapshot_bytes / _tag,
qvc_stream_export_slots / _import_slots; csrc/qvc_stream.h: SnapLayout, move_slots): what a stream is between two calls --
the kept 2*H frames of its rows of every ring, pos and len -- cut out of one state and continued in any slot of another,
whatever the batch size and the hop.  The surface, the tag and the status codes on the product library; the rest through
the CPU twin of the drivers (tools/emu_twin.cpp: the same helper on the host copy backend, pointer form of the noise):

  P4  export, fill the whole state with 0xFF, import: every later output is torch.equal to the untouched run's;
  P5  a stream moved into another slot of its own run is torch.equal to the unmoved one, call by call; the freed slot
      takes a new stream;
  P6  3 slots hop 4 -> 1 slot hop 5 at pos 11, and 1 slot hop 5 -> a busy 3-slot hop-4 run at pos 13: the moved stream and
      its new neighbours against the emulation's own whole-utterance conversion, >= 90 dB (bit equality is printed);
  P7  a slot that never stepped, and a stream that has ended and is flushing;
  P8  byte for byte what an export and an import touch.

Shapes: rows up16_k17_up2_k2 and mb_up16_up1 with the WaveNet (2, 1, 2), 3 slots or 1, hops 4 and 5, streams of
37 / 23 / 9 frames (tests/snapshot_common.py has the scenarios, shared with tests/test_gpu_stream_snapshot.py).
"""
import ctypes
import functools
import os
import re

import pytest
import torch

import config_space as CS
import snapshot_common as SN
import stream_tick_common as SC
from helpers import ROOT
from live_common import built, twin_library  # noqa: F401
from stream_tick_common import LENS, ROW, ROW_MB

NEW = ("qvc_stream_snapshot_bytes", "qvc_stream_snapshot_tag", "qvc_stream_export_slots", "qvc_stream_import_slots")


@pytest.fixture(scope="module")
def twin(built):
    return SN.declare_twin(twin_library())


@functools.lru_cache(maxsize=None)
def _whole(name):
    """The emulated whole-utterance conversion of the row's three streams; computed once, read-only."""
    from emu import emu_infer_ragged
    mc, sd = SC.row_problem(name)
    unit, g, noise = SC.row_inputs(name)
    return emu_infer_ragged(mc, sd, unit, g, noise, LENS)


def _make(built, twin, name):
    mc, sd = SC.row_problem(name)
    _unit, g, _noise = SC.row_inputs(name)
    return lambda B, hop: SN.TwinSnapRunner(built, twin, mc, sd, g, B, hop)


def _cfg(name=ROW, wn=SC.WN, dtype="f16"):
    from quickvc_official_amd import lib as L
    mc, _sd = SC.row_problem(name, wn)
    return L.make_config(dict(mc, operand_dtype=dtype))


def _tag(built, cfg):
    tag = ctypes.c_uint64(0)
    assert built.qvc_stream_snapshot_tag(ctypes.byref(cfg), ctypes.byref(tag)) == 0
    return int(tag.value)


# ---------------------------------------------------------------- P1
def test_surface(built, twin):
    header = open(os.path.join(ROOT, "include", "qvc.h")).read()
    for name in NEW:
        assert hasattr(built, name), name
        assert re.search(r"\b%s\(" % name, header), name
    assert built.qvc_abi_version() == 8 and "#define QVC_ABI_VERSION 8" in header
    assert hasattr(twin, "qvc_emu_stream_export_slots") and hasattr(twin, "qvc_emu_stream_import_slots")


@pytest.mark.parametrize("name", [ROW, ROW_MB])
def test_snapshot_size(built, twin, name):
    """One size per model: positive, a multiple of 256, the carved sum of rows * keep over the ring table plus pos and len
    -- the same from the table of every (batch, hop)."""
    cfg = _cfg(name)
    n = int(built.qvc_stream_snapshot_bytes(ctypes.byref(cfg)))
    assert n > 0 and n % 256 == 0
    for B, hop in ((1, 4), (3, 4), (3, 5), (2, 320)):
        table = SC.ring_table(twin, cfg, B, hop)
        for per in table:
            assert SN.layout_bytes(per) == n, (B, hop)
        assert n < int(built.qvc_stream_state_bytes(ctypes.byref(cfg), 1, hop)) + 256


# ---------------------------------------------------------------- P2
def test_tag(built):
    base = _tag(built, _cfg())
    assert base == _tag(built, _cfg()) and base != 0
    others = {"the other row": _cfg(ROW_MB), "bf16": _cfg(dtype="bf16"), "WaveNet (3, 1, 2)": _cfg(wn=(3, 1, 2))}
    tags = {k: _tag(built, c) for k, c in others.items()}
    assert len({base, *tags.values()}) == 4, (base, tags)
    assert built.qvc_stream_snapshot_tag(ctypes.byref(_cfg()), None) == -1 and built.qvc_stream_snapshot_tag(None, ctypes.byref(ctypes.c_uint64())) == -1


# ---------------------------------------------------------------- P3
def test_status_codes(built):
    """Every refusal, in the stated order.  None of these calls gets as far as a launch: every pointer is checked (never
    followed) on the host first."""
    import quickvc_official_amd as q
    from quickvc_official_amd import lib as L
    cfg = _cfg()
    p = ctypes.byref(cfg)
    single = L.make_config(q.SynthesizerTrn(641, 32, **q.ISTFT_MODEL_CONFIG).model_config)
    one_up = L.make_config(CS.problem("one_up8")[1])
    assert int(single.n_ups) == 2 and int(one_up.n_ups) == 1
    size = built.qvc_stream_snapshot_bytes
    assert size(None) == -1 and size(ctypes.byref(single)) == -2 and size(ctypes.byref(one_up)) == -2
    tag = ctypes.c_uint64(0)
    assert built.qvc_stream_snapshot_tag(ctypes.byref(single), ctypes.byref(tag)) == -2
    assert built.qvc_stream_snapshot_tag(ctypes.byref(one_up), ctypes.byref(tag)) == -2
    n_state, n_snap = int(built.qvc_stream_state_bytes(p, 3, 5)), int(size(p))
    a = 1 << 20                                                            # any 256-byte aligned non-null address
    for fn in (built.qvc_stream_export_slots, built.qvc_stream_import_slots):
        def call(cfg_=cfg, state=a, ns=n_state, B=3, hop=5, slots=(0, 2), n=None, pos=a, ln=a, snap=a, nb=2 * n_snap):
            arr = None if slots is None else SN.slot_array(slots)
            return fn(None if cfg_ is None else ctypes.byref(cfg_), state, ns, B, hop, arr, len(slots or ()) if n is None else n, pos, ln, snap, nb, None)
        # 1. pointers, counts, slots
        for null in ("cfg_", "state", "pos", "ln", "snap", "slots"):
            assert call(**{null: None}, **({"n": 2} if null == "slots" else {})) == -1, null
        assert call(B=0) == -1 and call(B=-1) == -1 and call(n=0) == -1 and call(n=-3) == -1
        assert call(slots=(0, 3)) == -1 and call(slots=(-1,)) == -1 and call(slots=(1,), B=1) == -1
        # 2. the plan
        assert call(hop=0) == -1 and call(hop=-2) == -1
        assert call(cfg_=single) == -2 and call(cfg_=one_up) == -2
        # 3. the sizes
        assert call(ns=n_state - 1) == -5 and call(nb=2 * n_snap - 1) == -5 and call(slots=(0, 1, 2), nb=2 * n_snap) == -5
        # 4. the alignments (the step's code for a misaligned state)
        assert call(state=a + 4) == -1 and call(snap=a + 16) == -1
        # the order: 1 in front of 2 in front of 3 in front of 4
        assert call(slots=(0, 3), cfg_=single) == -1 and call(B=0, cfg_=single, ns=1) == -1
        assert call(cfg_=single, ns=1) == -2 and call(cfg_=one_up, nb=1, state=a + 4) == -2
        assert call(hop=0, ns=1) == -1
        assert call(ns=1, state=a + 4) == -5 and call(nb=1, snap=a + 4) == -5


# ---------------------------------------------------------------- P4 - P8
@pytest.mark.parametrize("name,hop", [(ROW, 4), (ROW, 5), (ROW_MB, 5)])
def test_round_trip_through_a_wiped_state(built, twin, name, hop):
    SN.round_trip(_make(built, twin, name), name, hop)


@pytest.mark.parametrize("name,hop", [(ROW, 4), (ROW_MB, 5)])
def test_another_slot_same_geometry(built, twin, name, hop):
    SN.same_geometry(_make(built, twin, name), name, hop, _whole(name))


@pytest.mark.parametrize("name", [ROW, ROW_MB])
def test_to_one_slot_and_another_hop(built, twin, name):
    SN.to_one_slot(_make(built, twin, name), name, _whole(name))


@pytest.mark.parametrize("name", [ROW, ROW_MB])
def test_into_a_busy_run_of_another_hop(built, twin, name):
    SN.to_three_slots(_make(built, twin, name), name, _whole(name))


@pytest.mark.parametrize("s,calls_before", [(0, 0), (2, 3)])
def test_edges(built, twin, s, calls_before):
    SN.edge(_make(built, twin, ROW), ROW, _whole(ROW), s, calls_before)


@pytest.mark.parametrize("name", [ROW, ROW_MB])
def test_exactly_what_is_touched(built, twin, name):
    SN.touched(_make(built, twin, name), name)


def test_twin_refuses_as_the_library(built, twin):
    """The twin runs the same checks (snapshot_slots): a slot out of range, a short snapshot buffer, nothing written."""
    R = _make(built, twin, ROW)(3, 4)
    for b in range(3):
        R.idle(b)
    before = R.state()
    _raw, snap = SC._aligned(R.n_snap, 0xEE)
    args = (R.p, R._state.data_ptr(), R.n_state, 3, 4)
    tail = (R._pos.data_ptr(), R._len.data_ptr(), snap.data_ptr())
    for fn in (twin.qvc_emu_stream_export_slots, twin.qvc_emu_stream_import_slots):
        assert fn(*args, SN.slot_array([3]), 1, *tail, R.n_snap) == -1
        assert fn(*args, SN.slot_array([0, 1]), 2, *tail, R.n_snap) == -5
        assert fn(*args[:3], 3, 0, SN.slot_array([0]), 1, *tail, R.n_snap) == -1
    assert torch.equal(R.state(), before) and bool((snap == 0xEE).all())


# ---------------------------------------------------------------- the byte form (no device involved)
def test_snapshot_bytes_round_trip():
    from quickvc_official_amd.streaming import StreamSnapshot
    data = torch.arange(512, dtype=torch.int32).to(torch.uint8)
    for rng in (None, (0x5EED1234ABCD, 0.75)):
        snap = StreamSnapshot(0xFEDCBA9876543210, data, torch.randn(7), 0x9E3779B97F4A7C15, 11, 37, rng)
        back = StreamSnapshot.frombytes(snap.cpu().tobytes())
        assert (back.tag, back.key, back.position, back.length, back.rng) == (snap.tag, snap.key, 11, 37, rng)
        assert torch.equal(back.data, data) and torch.equal(back.g, snap.g)
    raw = snap.tobytes()
    for bad in (raw[:-1], b"x" + raw[1:], raw[:10]):
        with pytest.raises(ValueError):
            StreamSnapshot.frombytes(bad)
