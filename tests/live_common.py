"""What the four test files of the windowed step and its tick form share (tests/test_gpu_live.py, test_gpu_live_tick.py,
test_live_host.py, test_live_tick_host.py): fixtures -- imported by name into the module that uses them -- and helpers."""
import ctypes
import functools
import sys

import pytest
import torch

import config_space as CS
from helpers import ROOT

DEBUG_DEFAULTS = {"post_tail": 1, "post_tail_nf": 4, "pair_wide_launch": 1, "pair_cm4": 1, "conv_cl": 1, "wn_chunk": 0,
                  "pair_chain3": 0, "wn_kernel": 0, "launch_stop": -1, "live_trim": 1}
NAN = float("nan")
SEED = 0x5EED1234ABCD


# ---------------------------------------------------------------- the host files
@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from quickvc_official_amd import lib as L
    return L.load_library()


def twin_library():
    """oracle/_build/libqvc_emu_twin.so (tools/emu_twin.cpp), its lockstep and tick exports declared."""
    import importlib
    from quickvc_official_amd import lib as L
    lib = ctypes.CDLL(importlib.import_module("quickvc_official_amd.build").build_emu_twin())
    P, I, Lg, V = ctypes.POINTER, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    lib.qvc_emu_live_step.restype = ctypes.c_int
    lib.qvc_emu_live_step.argtypes = [P(L.QvcConfig), V, V, Lg, V, V, V, V, I, I, I, V, V, V, Lg]
    lib.qvc_emu_live_tick.restype = ctypes.c_int
    lib.qvc_emu_live_tick.argtypes = [P(L.QvcConfig), V, V, Lg, V, V, V, V, I, I, I, V, V, V, V, Lg]
    for reset in (lib.qvc_emu_live_reset_slot, lib.qvc_emu_live_tick_reset_slot):
        reset.restype = ctypes.c_int
        reset.argtypes = [P(L.QvcConfig), V, Lg, I, I, I, I, I, V, V]
    lib.qvc_emu_live_tick_ring.restype = ctypes.c_int
    lib.qvc_emu_live_tick_ring.argtypes = [P(L.QvcConfig), I, I, I, I, I, P(Lg), P(Lg)]
    for trim in (lib.qvc_emu_live_trim, lib.qvc_emu_live_tick_trim):
        trim.restype = None
        trim.argtypes = [I]
    return lib


def _context(built, cfg):
    return int(built.qvc_live_context_frames(ctypes.byref(cfg)))


def _spf(cfg):
    n = int(cfg.hop) * int(cfg.subbands)
    for i in range(int(cfg.n_ups)):
        n *= int(cfg.upsample_rates[i])
    return n


def _aligned(n, fill):
    raw = torch.full((n + 256,), fill, dtype=torch.uint8)
    shift = (-raw.data_ptr()) % 256
    return raw, raw[shift:shift + n]


# ---------------------------------------------------------------- the GPU files
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from quickvc_official_amd import lib as L
    l = L.load_library()                       # raises if the HIP library is missing: no fallback
    assert l.qvc_device_check() == 0
    return l


@pytest.fixture(autouse=True)
def _debug_switches_at_defaults():
    from quickvc_official_amd import lib as L
    for k, v in DEBUG_DEFAULTS.items():
        L.debug_set(k, v)
    yield
    for k, v in DEBUG_DEFAULTS.items():
        L.debug_set(k, v)


class _Model:
    """What the converters need of a model, for configurations SynthesizerTrn's constructor cannot name (the WaveNet keys)."""

    def __init__(self, mc, sd, dev, dtype="f16"):
        from quickvc_official_amd.engine import QvcEngine
        self.model_config = dict(mc, operand_dtype=dtype)
        self._engine = QvcEngine(self.model_config, sd, dev)
        self.samples_per_frame = self._engine.samples_per_frame

    def engine(self):
        return self._engine


@functools.lru_cache(maxsize=None)
def _row_model(name, wn=None, dtype="f16", sizes="live_sizes"):
    """(model, C) of a row of the configuration space; wn = (enc_layers, flow_layers, n_flows): the row with that WaveNet
    geometry (kernel 5) and weights from wn_state_dict -- a short WaveNet keeps the window small.  sizes: the engine's
    query that reports C ("live_sizes" | "live_tick_sizes")."""
    cfg, mc, sd = CS.problem(name)
    if wn is not None:
        keys = dict(wn_kernel_size=5, enc_layers=wn[0], flow_layers=wn[1], n_flows=wn[2])
        cfg, mc = dict(cfg, **keys), dict(mc, **keys)
        sd = CS.wn_state_dict(dict(sd), cfg)
    model = _Model(mc, sd, torch.device("cuda:0"), dtype)
    return model, getattr(model.engine(), sizes)(1, 1, 0)[2]


def _keys(n):
    return [0x9E3779B97F4A7C15 * (i + 1) & 0xFFFFFFFFFFFFFFFF for i in range(n)]


def _prefix_rows(eng, unit_b, g_b, noise_b, key, prefixes, min_frames=0):
    """The conversions of the prefixes of ONE stream, as rows of one ragged call -> (len(prefixes), 1, max * spf); the
    call is at least min_frames wide."""
    R, t = len(prefixes), max(max(prefixes), min_frames)
    frames = torch.tensor(prefixes, dtype=torch.int32)
    u, gg = unit_b[None, :, :t].expand(R, -1, -1).contiguous(), g_b[None].expand(R, -1).contiguous()
    if noise_b is None:
        return eng.infer_batch_ragged(u, gg, None, frames, rng=(SEED, [key] * R, 1.0)).clone()
    return eng.infer_batch_ragged(u, gg, noise_b[None, :, :t].expand(R, -1, -1).contiguous(), frames).clone()
