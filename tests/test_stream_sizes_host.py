"""CPU tests (no GPU) that pin what the ring table of csrc/qvc_stream.h must not change:

  sizes     the state / workspace bytes, lags and context of the three streaming forms, and the byte range of every
            slot's rings in the tick state, against tests/golden/stream_sizes.json (written by
            tests/golden/make_golden_stream_sizes.py before the rings were stated in one table);
  launches  how one step of every driver groups its copies into launches (copy_batch and copy_counted calls and their
            descriptors), counted by the CPU twin's counting backend (tools/emu_twin.cpp).
"""
import ctypes
import importlib.util
import json
import os

import pytest
import torch

from helpers import ROOT
from live_common import _aligned, built, twin_library  # noqa: F401


@pytest.fixture(scope="module")
def twin(built):
    return twin_library()


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_stream_sizes", os.path.join(ROOT, "tests", "golden", "make_golden_stream_sizes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sizes_and_ring_ranges_match_the_golden_table(built, twin):
    gen = _generator()
    want = json.load(open(gen.PATH))
    got = gen.collect(built, twin)
    assert sorted(got) == sorted(want) == sorted(gen.SHIPPED + gen.ROWS)
    accepted = refused = 0
    for name in want:
        assert sorted(got[name]) == sorted(want[name]), name
        for field in want[name]:
            assert got[name][field] == want[name][field], (name, field)
        for key, (state, ws) in want[name]["tick"].items():
            accepted += state > 0
            refused += want[name]["stream"][key.rsplit(",", 1)[0]][0] < 0
    assert accepted == len(want) * 18 and refused > 0      # every (B, hop, L) of the windowed forms; the segment rings refuse some rows


def launch_counts(built, twin):
    """{case: [copy_batch calls, descriptors, 0, 0]} of ONE step of each driver on MINI_MODEL_CONFIG: 2 streams, hop 4,
    look-ahead 2, pointer form of the noise, zeroed state (the last two words counted the launches of the tick's own ring
    mechanism, which is gone; the rows keep their shape); under "counted", [copy_counted calls, descriptors] of the tick."""
    import quickvc_official_amd as q
    from quickvc_official_amd import lib as L
    from quickvc_official_amd.synth import make_synthetic_inputs, make_synthetic_state_dict
    model = q.SynthesizerTrn(641, 32, **q.MINI_MODEL_CONFIG)
    mc, sd = model.model_config, make_synthetic_state_dict(model, 1234)
    cfg = L.make_config(dict(mc, operand_dtype="f16"))
    p = ctypes.byref(cfg)
    blob = L.pack_weights(built, cfg, sd)
    B, hop, look = 2, 4, 2
    unit, g, noise = make_synthetic_inputs(B, hop, 256, mc["inter_channels"], mc["gin_channels"], seed0=8900)
    unit, g, noise = unit.contiguous(), g.float().contiguous(), noise.contiguous()
    spf = int(cfg.hop) * int(cfg.subbands) * int(cfg.upsample_rates[0]) * int(cfg.upsample_rates[1])
    lens = torch.full((B,), 1 << 20, dtype=torch.int32)
    n_new = torch.full((B,), hop, dtype=torch.int32)
    I, Lg, V = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    twin.qvc_emu_twin_stream_step.restype = ctypes.c_int
    twin.qvc_emu_twin_stream_step.argtypes = [ctypes.POINTER(L.QvcConfig), V, V, Lg, V, V, V, V, I, I, V, V, V, Lg]
    twin.qvc_emu_twin_counts.restype = None
    twin.qvc_emu_twin_counts.argtypes = [ctypes.POINTER(Lg)]
    twin.qvc_emu_stream_tick_counts.restype = None
    twin.qvc_emu_stream_tick_counts.argtypes = [ctypes.POINTER(Lg)]

    def run(call, n_state, n_ws):
        assert n_state > 0 and n_ws > 0
        _k1, state = _aligned(n_state, 0)
        _k2, ws = _aligned(n_ws, 0)
        pos = torch.zeros(B, dtype=torch.int32)
        out = torch.zeros(B, hop * spf)
        twin.qvc_emu_twin_counts(None)
        assert call(state, n_state, ws, n_ws, pos, out) == 0
        counts = (Lg * 4)()
        twin.qvc_emu_twin_counts(counts)
        return list(counts)

    def stream(state, ns, ws, nw, pos, out):
        return twin.qvc_emu_twin_stream_step(p, blob.data_ptr(), state.data_ptr(), ns, unit.data_ptr(), g.data_ptr(), noise.data_ptr(),
                                             out.data_ptr(), B, hop, pos.data_ptr(), lens.data_ptr(), ws.data_ptr(), nw)

    def step(state, ns, ws, nw, pos, out):
        return twin.qvc_emu_live_step(p, blob.data_ptr(), state.data_ptr(), ns, unit.data_ptr(), g.data_ptr(), noise.data_ptr(),
                                      out.data_ptr(), B, hop, look, pos.data_ptr(), lens.data_ptr(), ws.data_ptr(), nw)

    def tick(state, ns, ws, nw, pos, out):
        return twin.qvc_emu_live_tick(p, blob.data_ptr(), state.data_ptr(), ns, unit.data_ptr(), g.data_ptr(), noise.data_ptr(),
                                      out.data_ptr(), B, hop, look, n_new.data_ptr(), pos.data_ptr(), lens.data_ptr(), ws.data_ptr(), nw)
    live = (int(built.qvc_live_state_bytes(p, B, hop, look)), int(built.qvc_live_workspace_bytes(p, B, hop, look)))
    got = {"stream_step": run(stream, int(built.qvc_stream_state_bytes(p, B, hop)), int(built.qvc_stream_workspace_bytes(p, B, hop)))}
    twin.qvc_emu_live_trim(1)
    got["live_step trimmed"] = run(step, *live)
    twin.qvc_emu_stream_tick_counts(None)
    got["live_tick trimmed"] = run(tick, int(built.qvc_live_tick_state_bytes(p, B, hop, look)), int(built.qvc_live_tick_workspace_bytes(p, B, hop, look)))
    counted = (Lg * 2)()
    twin.qvc_emu_stream_tick_counts(counted)
    got["counted"] = list(counted)
    twin.qvc_emu_live_trim(0)
    got["live_step plain"] = run(step, *live)
    twin.qvc_emu_live_trim(1)
    return got


# Obtained at the commit before the ring table: this file's launch_counts() on the same counting backend compiled against
# that commit's csrc/qvc_stream.h.  They are not derived from the present drivers.
# The tick's row since live_step and live_tick are one body: the two trimmed hand-offs stay copy_batch over all slots,
# [2, 2]; what a step moves beside them is "live_step plain", [3, 7], recorded as said above -- append (2 descriptors in
# the pointer form), deliver plus the two kept parts out (3), the two kept parts back in (2) -- and those three launches
# are, by construction, the tick's own through copy_counted: "counted".
LAUNCHES = {
    "stream_step": [9, 39, 0, 0],
    "live_step trimmed": [5, 9, 0, 0],
    "live_step plain": [3, 7, 0, 0],
    "live_tick trimmed": [2, 2, 0, 0],
}
LAUNCHES["counted"] = LAUNCHES["live_step plain"][:2]


def test_launch_grouping_of_one_step(built, twin):
    got = launch_counts(built, twin)
    print(got)
    assert got == LAUNCHES
