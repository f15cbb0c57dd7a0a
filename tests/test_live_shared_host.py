"""CPU tests (no GPU) of the SHARED rule of the window's rings (csrc/qvc_stream.h: live_rings, live_run): qvc_live_step and
qvc_live_tick are one body on two movers and keep one ring layout, so they may alternate on one state.  Through the CPU
twin (tools/emu_twin.cpp), pointer form of the noise; the scenarios are tests/live_shared_common.py's, the GPU runs them in
tests/test_gpu_live_shared.py."""
import ctypes

import pytest
import torch

import live_shared_common as SC
from live_common import _aligned, _context, _spf, built, twin_library  # noqa: F401


class TwinCalls:
    device = torch.device("cpu")

    def __init__(self, built, twin, mc, sd):
        from quickvc_official_amd import lib as L
        self.built, self.twin = built, twin
        self.cfg = L.make_config(dict(mc, operand_dtype="f16"))
        self.p = ctypes.byref(self.cfg)
        self.blob = L.pack_weights(built, self.cfg, sd)
        self.context = _context(built, self.cfg)
        self.spf = _spf(self.cfg)

    def sizes(self, B, hop, L_, tick):
        ws = self.built.qvc_live_tick_workspace_bytes if tick else self.built.qvc_live_workspace_bytes
        state = self.built.qvc_live_tick_state_bytes if tick else self.built.qvc_live_state_bytes
        return int(state(self.p, B, hop, L_)), int(ws(self.p, B, hop, L_))

    def buffer(self, n):
        self._keep = getattr(self, "_keep", []) + [_aligned(n, 0xFF)]
        return self._keep[-1][1]

    def reset(self, state, B, hop, L_, slot, length, pos, lens):
        assert self.twin.qvc_emu_live_reset_slot(self.p, state.data_ptr(), state.numel(), B, hop, L_, slot, length, pos.data_ptr(), lens.data_ptr()) == 0

    def step(self, state, ws, u, g, nz, out, pos, lens, L_):
        B, hop = u.shape[0], u.shape[2]
        assert self.twin.qvc_emu_live_step(self.p, self.blob.data_ptr(), state.data_ptr(), state.numel(), u.data_ptr(), g.data_ptr(), nz.data_ptr(),
                                           out.data_ptr(), B, hop, L_, pos.data_ptr(), lens.data_ptr(), ws.data_ptr(), ws.numel()) == 0

    def tick(self, state, ws, u, g, nz, out, n_new, pos, lens, L_):
        B, hop = u.shape[0], u.shape[2]
        assert self.twin.qvc_emu_live_tick(self.p, self.blob.data_ptr(), state.data_ptr(), state.numel(), u.data_ptr(), g.data_ptr(), nz.data_ptr(),
                                           out.data_ptr(), B, hop, L_, n_new.data_ptr(), pos.data_ptr(), lens.data_ptr(), ws.data_ptr(), ws.numel()) == 0

    def ring(self, B, hop, L_, slot, which):
        return SC.twin_ring(self.twin, self.cfg, B, hop, L_, slot, which)


@pytest.fixture(scope="module")
def twin(built):
    lib = twin_library()
    yield lib
    lib.qvc_emu_live_trim(1)


@pytest.fixture(scope="module")
def problem(built, twin):
    mc, sd, unit, g, noise = SC.mini_problem(9600)
    return TwinCalls(built, twin, mc, sd), unit, g, noise


@pytest.mark.parametrize("trim", [1, 0], ids=["trimmed", "plain"])
@pytest.mark.parametrize("hop", [4, 5])
def test_twin_steps_and_ticks_share_one_state(problem, twin, hop, trim):
    calls, unit, g, noise = problem
    twin.qvc_emu_live_trim(trim)
    SC.check_shared_state(calls, unit, g, noise, hop, calls.spf, seed=9700 + hop)


@pytest.mark.parametrize("trim", [1, 0], ids=["trimmed", "plain"])
@pytest.mark.parametrize("hop", [4, 5])
def test_twin_state_after_ragged_ticks(problem, twin, hop, trim):
    calls, unit, g, noise = problem
    twin.qvc_emu_live_trim(trim)
    SC.check_state_after_ragged_ticks(calls, unit, g, noise, hop, calls.spf)


def test_a_backend_without_the_hook_is_refused(problem, twin):
    """live_tick on the frozen emulation's backend, which states no kStreamTick: QVC_ERR_BAD_CONFIG, for a geometry the
    twin's own backend accepts (the sibling of qvc_emu_stream_tick_frozen)."""
    from quickvc_official_amd import lib as L
    calls, _unit, _g, _noise = problem
    twin.qvc_emu_live_tick_frozen.restype = ctypes.c_int
    twin.qvc_emu_live_tick_frozen.argtypes = [ctypes.POINTER(L.QvcConfig), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    assert calls.sizes(2, 4, 2, True)[1] > 0
    assert twin.qvc_emu_live_tick_frozen(calls.p, 2, 4, 2) == -2
    assert twin.qvc_emu_live_tick_frozen(calls.p, 2, 0, 2) == -1          # the plan's refusal comes first
