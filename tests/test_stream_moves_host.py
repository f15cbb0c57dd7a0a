"""CPU test (no GPU) that pins the WORK of the segment rings' two calls (csrc/qvc_stream.h: stream_step, stream_tick): every
copy_batch / copy_counted launch of one call, descriptor by descriptor -- pointers as (buffer, byte offset), every numeric
field, the flags and a tick's bookkeeping head --, recorded by the CPU twin's recording backend (tools/emu_twin.cpp:
qvc_emu_stream_moves), equals tests/golden/stream_moves.json.  That file was written by
tests/golden/make_golden_stream_moves.py while the two drivers were still two hand-written bodies; bit-equal outputs show
that the values are right, this shows that the GPU is handed the same moves.
"""
import importlib.util
import json
import os

import pytest

from helpers import ROOT
from live_common import built, twin_library  # noqa: F401


@pytest.fixture(scope="module")
def twin(built):
    return twin_library()


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_stream_moves", os.path.join(ROOT, "tests", "golden", "make_golden_stream_moves.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_move_is_the_golden_one(built, twin):
    gen = _generator()
    want = json.load(open(gen.PATH))
    got = json.loads(json.dumps(gen.collect(built, twin)))
    assert sorted(got) == sorted(want) and len(want) == 2 * 2 * 3 + 2
    for case in sorted(want):
        assert len(got[case]) == len(want[case]), (case, "launches")
        for i, (g, w) in enumerate(zip(got[case], want[case])):
            assert g["op"] == w["op"] and g.get("head") == w.get("head"), (case, i, g.get("head"), w.get("head"))
            assert len(g["descs"]) == len(w["descs"]), (case, i, "descriptors")
            for j, (gd, wd) in enumerate(zip(g["descs"], w["descs"])):
                assert gd == wd, (case, i, j, gd, wd)
    # what the table must hold: the step's launches are copy_batch, a tick's copy_counted, the same number of them, and a
    # step spends one descriptor more than a tick (the zero fill behind the noise)
    for case, calls in want.items():
        assert {c["op"] for c in calls} == ({"copy_batch"} if case.endswith("step") else {"copy_counted"}), case
    for case in want:
        if not case.endswith("step"):
            step = want[case.split(" tick")[0] + " step"]
            assert len(want[case]) == len(step), case
            assert sum(len(c["descs"]) for c in step) == sum(len(c["descs"]) for c in want[case]) + 1, case
