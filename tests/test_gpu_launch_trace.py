"""GPU test (run with -m gpu) that ties the host's selection trace to what the library dispatches: the record names of
qvc_infer_batch_timed -- TimedBackend builds them from the LaunchChoice of every launch (csrc/qvc_api.hip) -- are exactly
the names built from the CPU twin's selection trace of the same call (tools/emu_twin.cpp: qvc_emu_launch_trace;
tests/golden/make_golden_launch_trace.py: record_names).  tests/test_launch_trace_host.py pins the twin's choices without
a GPU; this shows that the library on the GPU makes the same ones.

Cases: MINI_MODEL_CONFIG (4-wave pairs) and the rows init768 and init1024 of tests/config_space.py (8-wave pairs of three
and of four fragments) at that file's small shape, B 2, T 23, in f16; the shipped configuration at B 1, T 64 in bf16x.
"""
import ctypes
import importlib
import importlib.util
import os

import pytest
import torch

import config_space as CS
from helpers import ROOT

pytestmark = pytest.mark.gpu

CASES = [("MINI_MODEL_CONFIG", CS.B, CS.T, "f16"), ("init768", CS.B, CS.T, "f16"), ("init1024", CS.B, CS.T, "f16"), ("shipped", 1, 64, "bf16x")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from quickvc_official_amd import lib as L
    l = L.load_library()
    assert l.qvc_device_check() == 0
    return l


@pytest.fixture(scope="module")
def tracer():
    spec = importlib.util.spec_from_file_location("make_golden_launch_trace", os.path.join(ROOT, "tests", "golden", "make_golden_launch_trace.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    twin = gen.declare(ctypes.CDLL(importlib.import_module("quickvc_official_amd.build").build_emu_twin()))
    names, kinds = gen.layout(twin)
    return gen, twin, names, kinds


def _problem(name):
    """(model_config, state dict, inter channels, gin channels)"""
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_state_dict
    if name in CS.ROWS:
        cfg, mc, sd = CS.problem(name)
        return mc, sd, cfg["inter_channels"], cfg["gin_channels"]
    cfg = q.MINI_MODEL_CONFIG if name == "MINI_MODEL_CONFIG" else q.DEFAULT_MODEL_CONFIG
    model = q.SynthesizerTrn(641, 32, **cfg)
    return dict(model.model_config), make_synthetic_state_dict(model, CS.WEIGHTS_SEED), cfg["inter_channels"], cfg["gin_channels"]


@pytest.mark.parametrize("name,B,T,dtype", CASES)
def test_timed_records_are_named_by_the_selection_trace(lib, dev, tracer, name, B, T, dtype):
    from quickvc_official_amd.engine import QvcEngine
    from quickvc_official_amd.synth import make_synthetic_inputs
    gen, twin, names, kinds = tracer
    mc, sd, inter, gin = _problem(name)
    want = gen.record_names(gen.record(twin, kinds, mc, gen.PT.FORMS.index("uniform"), B, T, 1, gen.SWITCHES, dtype=dtype), names)
    unit, g, noise = make_synthetic_inputs(B, T, 256, inter, gin, seed0=CS.INPUTS_SEED)
    eng = QvcEngine(dict(mc, operand_dtype=dtype), sd, dev)
    _out, recs = eng.infer_batch_timed(unit.to(dev), g.to(dev), noise.to(dev))
    torch.cuda.synchronize()
    got = [r["name"] for r in recs]
    print(f"{name} B{B} T{T} {dtype}: {len(got)} launches: " + " ".join(got))
    assert len(want) > 10 and any(n.startswith("rbpair<") or n.startswith("conv<") for n in want)
    assert got == want
