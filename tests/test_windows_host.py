"""CPU tests (no GPU) of the exact windows over packed utterances (include/qvc.h: qvc_infer_windows_fm / _rng_fm;
csrc/qvc_stream.h: infer_windows): the C ABI's surface, sizes and refusals, the planner, and -- through the CPU twin of the
driver (tools/emu_twin.cpp: infer_windows on a backend derived from the frozen emulation's, the two table-driven kernels
restated in plain C++) -- what defines the call:

  * a row delivers the frames of the whole-utterance conversion of its utterance, for utterances of any lengths packed in
    one buffer and run in groups of rows, trimmed and plain;
  * nothing of out_packed but the delivered ranges is written;
  * the order of the table's rows changes no delivered sample;
  * no table content makes the call touch memory outside the caller's buffers.

Bar: >= 90 dB against the emulation's own whole-path result of the utterance alone (the project's bar for streamed
against offline; measured: bit equality).  The twin runs the pointer form only: the frozen emulation has no generator.
"""
import ctypes
import functools
import os
import re

import pytest
import torch

import config_space as CS
import memguard
from helpers import ROOT, snr_db
from live_common import _aligned, _context, _spf, built  # noqa: F401
from windows_common import NEW, SENTINEL, groups_of, mini_problem, packed_inputs, table_rows

LENGTHS, N, ROWS, EXTRA = (2, 16, 17, 89, 105, 200), 16, 3, 21


@functools.lru_cache(maxsize=None)
def _twin_lib():
    import importlib
    from quickvc_official_amd import lib as L
    lib = ctypes.CDLL(importlib.import_module("quickvc_official_amd.build").build_emu_twin())
    P, I, Lg, V = ctypes.POINTER, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    lib.qvc_emu_infer_windows_fm.restype = ctypes.c_int
    lib.qvc_emu_infer_windows_fm.argtypes = [P(L.QvcConfig), V, V, V, V, V, V, I, I, I, V, Lg]
    lib.qvc_emu_infer_windows_frozen.restype = ctypes.c_int
    lib.qvc_emu_infer_windows_frozen.argtypes = [P(L.QvcConfig), I, I]
    lib.qvc_emu_infer_batch_ragged_fm.restype = ctypes.c_int
    lib.qvc_emu_infer_batch_ragged_fm.argtypes = [P(L.QvcConfig), V, V, V, V, V, I, I, V, V, Lg]
    lib.qvc_emu_live_trim.restype = None
    lib.qvc_emu_live_trim.argtypes = [I]
    return lib


@pytest.fixture(scope="module")
def twin(built):
    lib = _twin_lib()
    yield lib
    lib.qvc_emu_live_trim(1)


def _mini_cfg():
    from quickvc_official_amd import lib as L
    mc, _sd = mini_problem()
    return L.make_config(dict(mc, operand_dtype="f16"))


# ---------------------------------------------------------------- the C ABI's surface
def test_exports_and_abi(built):
    header = open(os.path.join(ROOT, "include", "qvc.h")).read()
    for name in NEW:
        assert hasattr(built, name), name
        assert re.search(r"\b%s\(" % name, header), name
    assert "typedef struct qvc_window" in header
    assert built.qvc_abi_version() == 8 and "#define QVC_ABI_VERSION 8" in header


def test_sizes_are_positive_and_grow(built):
    import quickvc_official_amd as q
    from quickvc_official_amd import lib as L
    for name in ("DEFAULT_MODEL_CONFIG", "MINI_MODEL_CONFIG", "ISTFT_MODEL_CONFIG"):
        cfg = L.make_config(q.SynthesizerTrn(641, 32, **getattr(q, name)).model_config)
        p = ctypes.byref(cfg)
        C = _context(built, cfg)
        last = 0
        for rows, n in ((1, 1), (1, 16), (4, 16), (4, 256), (32, 256), (32, 1024)):
            w = int(built.qvc_windows_workspace_bytes(p, rows, n))
            assert w > 0 and w % 256 == 0 and w > last, (name, rows, n, w)
            last = w
            # the window's own scratch at hop n, look-ahead C is part of it, and so are the gathered windows
            assert w > int(built.qvc_live_tick_workspace_bytes(p, rows, n, C)) + rows * (2 * C + n) * 256 * 4, (name, rows, n)


def test_refusals_in_order(built):
    """Null pointers, rows < 1, window_frames < 1, total_frames < 1 and 2C + n > 1 << 24: -1; a bad plan: -2; a small
    workspace: -5; then the alignments: -1.  A call that breaks several rules reports the first.  None of these calls gets
    as far as a launch: every pointer is checked (never followed) on the host."""
    from quickvc_official_amd import lib as L
    cfg = _mini_cfg()
    p = ctypes.byref(cfg)
    C = _context(built, cfg)
    bad = CS.negative_config("n_flows_3")
    q = built.qvc_windows_workspace_bytes
    assert q(p, 0, 16) == -1 and q(p, -1, 16) == -1 and q(p, 4, 0) == -1 and q(p, 4, -5) == -1 and q(None, 4, 16) == -1
    assert q(p, 1, (1 << 24) - 2 * C + 1) == -1 and q(p, 1, (1 << 24) - 2 * C) > 0
    assert q(ctypes.byref(bad), 4, 16) == -2
    n_ws = int(q(p, 3, 16))
    a = 1 << 20                                                            # any 256-byte aligned non-null address
    rng = L.QvcNoiseRng(5, a, 1.0)

    def call(fn, draw, cfg_=cfg, blob=a, unit=a, win=a, g=a, out=a, rows=3, n=16, total=100, ws=a, nw=n_ws):
        return fn(ctypes.byref(cfg_), blob, unit, draw, win, g, out, rows, n, total, ws, nw, None)
    for fn, draw in ((built.qvc_infer_windows_fm, a), (built.qvc_infer_windows_rng_fm, ctypes.byref(rng))):
        for null in ("blob", "unit", "win", "g", "out", "ws"):
            assert call(fn, draw, **{null: None}) == -1, null
        assert call(fn, None) == -1
        assert call(fn, draw, rows=0) == -1 and call(fn, draw, n=0) == -1 and call(fn, draw, total=0) == -1
        assert call(fn, draw, n=(1 << 24) - 2 * C + 1, nw=1 << 62) == -1
        assert call(fn, draw, cfg_=bad) == -2
        assert call(fn, draw, nw=n_ws - 1) == -5 and call(fn, draw, n=17) == -5 and call(fn, draw, rows=4) == -5
        assert call(fn, draw, ws=a + 4) == -1 and call(fn, draw, blob=a + 4) == -1
        # the order: arguments before the plan, the plan before the size, the size before the alignment
        assert call(fn, draw, cfg_=bad, rows=0) == -1 and call(fn, draw, cfg_=bad, nw=0) == -2 and call(fn, draw, nw=0, ws=a + 4) == -5
    assert call(built.qvc_infer_windows_rng_fm, ctypes.byref(type(rng)(5, None, 1.0))) == -1


def test_a_backend_without_the_hook_is_refused(twin):
    cfg = _mini_cfg()
    assert twin.qvc_emu_infer_windows_frozen(ctypes.byref(cfg), 3, 16) == -2


def test_plan_windows_covers_every_frame_once():
    from quickvc_official_amd.windows import plan_windows
    lengths, n = [2, 15, 16, 17, 33], 16
    plan = plan_windows(lengths, n)
    seen = [[0] * length for length in lengths]
    for u, start, count in plan:
        assert 1 <= count <= n and 0 <= start and start + count <= lengths[u]
        for f in range(start, start + count):
            seen[u][f] += 1
    assert all(v == 1 for row in seen for v in row)
    assert len(plan) == 1 + 1 + 1 + 2 + 3
    with pytest.raises(ValueError):
        plan_windows(lengths, 0)


# ---------------------------------------------------------------- the CPU twin
@functools.lru_cache(maxsize=None)
def _problem():
    """cfg, blob and the packed problem: the utterances of LENGTHS back to back, then EXTRA frames that no row names."""
    from quickvc_official_amd import lib as L
    mc, sd = mini_problem()
    cfg = L.make_config(dict(mc, operand_dtype="f16"))
    blob = L.pack_weights(L.load_library(), cfg, sd)
    units, noise, g = packed_inputs(LENGTHS, mc["inter_channels"], mc["gin_channels"], 9100, extra=EXTRA)
    return cfg, blob, units, noise, g


def _table():
    """The plan's rows in order, one idle row with junk in its other fields put in explicitly (the 30 windows of LENGTHS
    fill ten groups of three exactly), and a g row per table row."""
    rows = table_rows(LENGTHS, N)
    owner = [u for u, length in enumerate(LENGTHS) for _ in range(-(-length // N))]
    at = len(rows) - 2                                    # inside the last group
    rows.insert(at, (7, 1 << 30, -3, 0))
    owner.insert(at, 0)
    return rows, owner


def _run(built, twin, rows, owner, trim, per=ROWS, arenas=None, table_override=None):
    """The table in groups of `per` rows through qvc_emu_infer_windows_fm on a workspace of NaN bytes -> out_packed, which
    starts as SENTINEL everywhere."""
    cfg, blob, units, noise, g = _problem()
    p = ctypes.byref(cfg)
    twin.qvc_emu_live_trim(1 if trim else 0)
    total, spf = units.shape[0], _spf(cfg)
    n_ws = int(built.qvc_windows_workspace_bytes(p, per, N))
    assert n_ws > 0
    if arenas is None:
        _keep, ws = _aligned(n_ws, 0xFF)
        out = torch.full((total * spf,), SENTINEL)
        u_in, n_in = units, noise
    else:
        ws = arenas.scratch("workspace", n_ws)
        out = arenas.output("out_packed", torch.float32, (total * spf,))
        u_in, n_in = arenas.input("unit_packed", units), arenas.input("noise_packed", noise)
    groups = groups_of(rows, per) if table_override is None else table_override
    g_rows = torch.zeros(groups.shape[0] * per, g.shape[1])
    g_rows[:len(owner)] = g[torch.tensor(owner)]
    for i in range(groups.shape[0]):
        tab = groups[i].contiguous() if arenas is None else arenas.input(f"table{i}", groups[i])
        gg = g_rows[i * per:(i + 1) * per].contiguous()
        st = twin.qvc_emu_infer_windows_fm(p, blob.data_ptr(), u_in.data_ptr(), n_in.data_ptr(), tab.data_ptr(), gg.data_ptr(), out.data_ptr(),
                                           per, N, total, ws.data_ptr(), n_ws)
        assert st == 0, (i, st)
    return out


@functools.lru_cache(maxsize=None)
def _alone(u):
    """The emulation's own whole-path conversion of utterance u alone, units frame-major; computed once, read-only."""
    from quickvc_official_amd import lib as L
    cfg, blob, units, noise, g = _problem()
    built, twin = L.load_library(), _twin_lib()
    base, T = sum(LENGTHS[:u]), LENGTHS[u]
    n_ws = int(built.qvc_workspace_bytes(ctypes.byref(cfg), 1, T))
    _keep, ws = _aligned(n_ws, 0x00)
    out = torch.full((T * _spf(cfg),), float("nan"))
    uu, nn, gg = units[base:base + T].contiguous(), noise[:, base:base + T].contiguous(), g[u:u + 1].contiguous()
    lens = torch.tensor([T], dtype=torch.int32)
    st = twin.qvc_emu_infer_batch_ragged_fm(ctypes.byref(cfg), blob.data_ptr(), uu.data_ptr(), gg.data_ptr(), nn.data_ptr(), out.data_ptr(), 1, T,
                                            lens.data_ptr(), ws.data_ptr(), n_ws)
    assert st == 0, st
    return out


@functools.lru_cache(maxsize=None)
def _trimmed_run():
    """out_packed of the whole table in the trimmed form; computed once, read-only."""
    from quickvc_official_amd import lib as L
    rows, owner = _table()
    return _run(L.load_library(), _twin_lib(), rows, owner, True)


def _check_utterances(out, spf):
    at = 0
    for u, length in enumerate(LENGTHS):
        got, want = out[at * spf:(at + length) * spf], _alone(u)
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(want).all()), u
        db = snr_db(want, got)
        print(f"utterance {u} ({length} frames): {db:.1f} dB")
        assert db >= 90.0, (u, db)
        at += length


@pytest.mark.parametrize("trim", [True, False], ids=["trimmed", "plain"])
def test_twin_windows_equal_the_utterance_alone(built, twin, trim):
    """Utterances of 2, 16, 17, 89, 105 and 200 frames in one packed buffer, n = 16, groups of 3 rows (an idle row among
    them): each utterance against the emulation's whole-path conversion of it alone."""
    cfg = _problem()[0]
    rows, owner = _table()
    out = _trimmed_run() if trim else _run(built, twin, rows, owner, False)
    _check_utterances(out, _spf(cfg))


def test_twin_writes_nothing_but_the_delivered_ranges(built, twin):
    """out_packed starts as a sentinel and holds EXTRA frames that no row names: they are still the sentinel, and the
    delivered ranges -- every other sample -- are not."""
    cfg = _problem()[0]
    out, spf = _trimmed_run(), _spf(cfg)
    named = sum(LENGTHS) * spf
    assert out.numel() == named + EXTRA * spf
    assert bool((out[named:] == SENTINEL).all())
    assert not bool((out[:named] == SENTINEL).any())
    # ... and a table that names part of an utterance leaves the rest of it alone
    rows = [r for r in table_rows(LENGTHS, N) if r[1] == 200 and r[2] in (0, 32, 192)]
    assert len(rows) == ROWS
    part = _run(built, twin, rows, [LENGTHS.index(200)] * ROWS, True)
    delivered = torch.zeros(out.numel(), dtype=torch.bool)
    for base, _length, start, count in rows:
        delivered[(base + start) * spf:(base + start + count) * spf] = True
    assert bool((part[~delivered] == SENTINEL).all()) and torch.equal(part[delivered], out[delivered])


def test_twin_row_order_changes_nothing(built, twin):
    """The table's rows shuffled -- other groups, other neighbours, other row numbers: bit for bit the same samples."""
    rows, owner = _table()
    perm = torch.randperm(len(rows), generator=torch.Generator().manual_seed(4)).tolist()
    assert perm != sorted(perm)
    shuffled = _run(built, twin, [rows[i] for i in perm], [owner[i] for i in perm], True)
    assert memguard.bits_equal(shuffled, _trimmed_run())


def test_twin_garbage_table_stays_inside_the_buffers(built, twin):
    """Negative and huge values in every field, every buffer in a guarded arena: no guard byte changes, no input changes,
    and what such a table delivers after clamping lies inside out_packed."""
    cfg = _problem()[0]
    big, small = (1 << 31) - 1, -(1 << 31)
    junk = [(small, big, small, big), (big, big, big, big), (-1, -1, -1, -1), (5, big, -7, big), (big, 3, 2, 1), (0, small, 0, 5),
            (3, 40, big, 16), (100, big, 17, small), (small, small, small, small)]
    arenas = memguard.ArenaSet("cpu", 0xFF, 0x5A)
    table = groups_of(junk, ROWS)
    out = _run(built, twin, junk, [0] * len(junk), True, arenas=arenas, table_override=table)
    assert arenas.check() == [], memguard.describe_guards(arenas.check())
    assert arenas.changed_inputs() == []
    assert out.numel() == _problem()[2].shape[0] * _spf(cfg)
