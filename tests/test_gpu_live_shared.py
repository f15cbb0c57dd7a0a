"""The SHARED rule of the window's rings on an MI355X (run with -m gpu): qvc_live_step and qvc_live_tick alternate on one
state.  The scenarios of tests/live_shared_common.py -- the CPU twin runs them in tests/test_live_shared_host.py -- through
QvcEngine's direct launches, in both noise forms and both forms of the step.  The ring offsets are the table's, asked of
the CPU twin (a host query)."""
import functools

import pytest
import torch

import live_shared_common as SC
from live_common import SEED, _Model, _debug_switches_at_defaults, _keys, dev, lib, twin_library  # noqa: F401

pytestmark = pytest.mark.gpu


class GpuCalls:
    def __init__(self, model, twin, device):
        self.eng, self.twin, self.device = model.engine(), twin, device
        self.context = self.eng.live_sizes(1, 1, 0)[2]
        self.spf = model.samples_per_frame
        self.keys = None                              # int64 device tensor: the generator form

    def sizes(self, B, hop, L_, tick):
        return (self.eng.live_tick_sizes if tick else self.eng.live_sizes)(B, hop, L_)[:2]

    def buffer(self, n):
        from quickvc_official_amd.engine import aligned_empty
        return aligned_empty(n, self.device).fill_(0xFF)

    def _rng(self, nz):
        return None if nz is not None else (SEED, self.keys, 1.0)

    def reset(self, state, B, hop, L_, slot, length, pos, lens):
        self.eng.live_reset_slot(state, B, hop, L_, slot, length, pos, lens)

    def step(self, state, ws, u, g, nz, out, pos, lens, L_):
        self.eng.live_step(state, ws, u, g, nz, out, pos, lens, L_, rng=self._rng(nz))

    def tick(self, state, ws, u, g, nz, out, n_new, pos, lens, L_):
        self.eng.live_tick(state, ws, u, g, nz, out, n_new, pos, lens, L_, rng=self._rng(nz))

    def ring(self, B, hop, L_, slot, which):
        return SC.twin_ring(self.twin, self.eng.cfg, B, hop, L_, slot, which)


@functools.lru_cache(maxsize=None)
def _problem():
    mc, sd, unit, g, noise = SC.mini_problem(9800)
    device = torch.device("cuda:0")
    calls = GpuCalls(_Model(mc, sd, device), twin_library(), device)
    calls.keys = torch.tensor([k - (1 << 64) if k >> 63 else k for k in _keys(len(SC.LENS))], dtype=torch.int64, device=device)
    return calls, unit, g.to(device), noise


def _case(form, trim):
    from quickvc_official_amd import lib as L
    calls, unit, g, noise = _problem()
    L.debug_set("live_trim", trim)                    # read when the step is issued; the launches here are direct
    return calls, unit, g, noise if form == "ptr" else None


@pytest.mark.parametrize("trim", [1, 0], ids=["trimmed", "plain"])
@pytest.mark.parametrize("form", ["ptr", "rng"])
@pytest.mark.parametrize("hop", [4, 5])
def test_steps_and_ticks_share_one_state(lib, dev, hop, form, trim):
    calls, unit, g, noise = _case(form, trim)
    SC.check_shared_state(calls, unit, g, noise, hop, calls.spf, seed=9700 + hop)


@pytest.mark.parametrize("trim", [1, 0], ids=["trimmed", "plain"])
@pytest.mark.parametrize("form", ["ptr", "rng"])
@pytest.mark.parametrize("hop", [4, 5])
def test_state_after_ragged_ticks(lib, dev, hop, form, trim):
    calls, unit, g, noise = _case(form, trim)
    SC.check_state_after_ragged_ticks(calls, unit, g, noise, hop, calls.spf)
