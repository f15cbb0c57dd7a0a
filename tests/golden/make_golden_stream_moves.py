#!/usr/bin/env python3
"""Generates tests/golden/stream_moves.json: every data-movement launch of one qvc_stream_step and one qvc_stream_tick,
descriptor by descriptor, as the CPU twin's recording backend sees them (tools/emu_twin.cpp: qvc_emu_stream_moves).

The file pins the WORK of the segment rings' two calls, not their values: it was written at commit 91072f1 ("Segment-ring
streams tick on their own"), the last one in which stream_step and stream_tick of csrc/qvc_stream.h were two hand-written
bodies, with the twin built against that commit's csrc/qvc_stream.h.  tests/test_stream_moves_host.py asserts that the
present drivers queue exactly these launches.  It is never regenerated: a change that is meant to move a descriptor
edits the file by hand and says why.

Per case, the calls in order.  A call is {"op": "copy_batch" | "copy_counted", "head": {...} (copy_counted only: slots,
hop, idle_pos and the six pointers of CountedHead), "descs": [every field of CopyDesc / CountedDesc]}.  A pointer is
[region, byte offset], region one of REGIONS: the buffer of the call it points into.  Descriptors do not depend on the
data, so one call per case is enough.  Pointer form of the noise (the emulation has no other).  Needs no GPU.

    python tests/golden/make_golden_stream_moves.py
"""
from __future__ import annotations

import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PATH = os.path.join(HERE, "stream_moves.json")
REGIONS = ("state", "workspace", "unit_new", "noise_new", "out", "pos", "lens", "n_new", "null")
HEAD_PTRS = ("n_new", "pos", "lens", "pos_eff", "len_eff", "pos_add")
BATCH_FIELDS = ("dpitch", "spitch", "width", "rows")
COUNTED_FIELDS = ("dpitch", "spitch", "fixed", "unit", "shift", "width", "rows", "flags")


def problems():
    """{model: (model_config, state dict, slots, hops)}: the two rows of tests/stream_tick_common.py with its short
    WaveNet, and MINI_MODEL_CONFIG as tests/test_stream_sizes_host.py::launch_counts runs it (four coupling layers: the
    work copy zwork[k & 1] alternates twice)."""
    import quickvc_official_amd as q
    import stream_tick_common as SC
    from quickvc_official_amd.synth import make_synthetic_state_dict
    out = {row: SC.row_problem(row) + (len(SC.LENS), SC.HOPS) for row in (SC.ROW, SC.ROW_MB)}
    model = q.SynthesizerTrn(641, 32, **q.MINI_MODEL_CONFIG)
    out["MINI_MODEL_CONFIG"] = (model.model_config, make_synthetic_state_dict(model, 1234), 2, (4,))
    return out


def calls_of(B, hop):
    """{name: counts (None: the step)} of the calls recorded per (model, hop)."""
    if B == 2:
        return {"step": None, "tick %d,0" % hop: [hop, 0]}
    return {"step": None, "tick 1,0,%d" % hop: [1, 0, hop], "tick %d,%d,%d" % (hop, hop, hop): [hop] * B}


def decode(words):
    """The recording's words (the layout RecordingBackend states in tools/emu_twin.cpp) -> the list of calls."""
    it = iter(words)

    def ptr():
        region, off = next(it), next(it)
        return [REGIONS[region], off]
    calls = []
    for op in it:
        n = next(it)
        call = {"op": ("copy_batch", "copy_counted")[op]}
        if op == 1:
            call["head"] = {k: next(it) for k in ("slots", "hop", "idle_pos")}
            call["head"].update({k: ptr() for k in HEAD_PTRS})
        fields = COUNTED_FIELDS if op == 1 else BATCH_FIELDS
        call["descs"] = [dict(dst=ptr(), src=ptr(), **{k: next(it) for k in fields}) for _ in range(n)]
        calls.append(call)
    return calls


def record(lib, twin, mc, sd, B, hop, counts):
    """One call on a zeroed state at position 0: the step (counts None) or the tick with these counts."""
    import torch
    from quickvc_official_amd import lib as L
    from quickvc_official_amd.synth import make_synthetic_inputs
    cfg = L.make_config(dict(mc, operand_dtype="f16"))
    p = ctypes.byref(cfg)
    blob = L.pack_weights(lib, cfg, sd)
    unit, g, noise = make_synthetic_inputs(B, hop, 256, mc["inter_channels"], mc["gin_channels"], seed0=8900)
    unit, g, noise = unit.float().contiguous(), g.float().contiguous(), noise.float().contiguous()
    spf = int(cfg.hop) * int(cfg.subbands) * int(cfg.upsample_rates[0]) * int(cfg.upsample_rates[1])
    n_state = int(lib.qvc_stream_state_bytes(p, B, hop))
    n_ws = int((lib.qvc_stream_workspace_bytes if counts is None else lib.qvc_stream_tick_workspace_bytes)(p, B, hop))
    assert n_state > 0 and n_ws > 0, (n_state, n_ws)
    state, ws = (torch.zeros(n + 256, dtype=torch.uint8) for n in (n_state, n_ws))
    state, ws = (t[(-t.data_ptr()) % 256:][:n] for t, n in ((state, n_state), (ws, n_ws)))
    pos = torch.zeros(B, dtype=torch.int32)
    lens = torch.full((B,), 1 << 20, dtype=torch.int32)
    n_new = None if counts is None else torch.tensor(counts, dtype=torch.int32)
    out = torch.zeros(B, hop * spf)
    cap = 1 << 16
    rec, used = (ctypes.c_int64 * cap)(), ctypes.c_int64(0)
    st = twin.qvc_emu_stream_moves(p, blob.data_ptr(), state.data_ptr(), n_state, unit.data_ptr(), g.data_ptr(), noise.data_ptr(), out.data_ptr(),
                                   B, hop, None if n_new is None else n_new.data_ptr(), pos.data_ptr(), lens.data_ptr(), ws.data_ptr(), n_ws,
                                   rec, cap, ctypes.byref(used))
    assert st == 0, ("qvc_emu_stream_moves", st)
    return decode(rec[:used.value])


def declare(twin):
    from quickvc_official_amd import lib as L
    I, Lg, V = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    twin.qvc_emu_stream_moves.restype = ctypes.c_int
    twin.qvc_emu_stream_moves.argtypes = [ctypes.POINTER(L.QvcConfig), V, V, Lg, V, V, V, V, I, I, V, V, V, V, Lg, ctypes.POINTER(Lg), Lg,
                                          ctypes.POINTER(Lg)]
    return twin


def collect(lib, twin):
    """{"<model> hop <hop> <call>": [calls]} from the product library `lib` (sizes, packer) and the CPU twin `twin`."""
    declare(twin)
    table = {}
    for name, (mc, sd, B, hops) in problems().items():
        for hop in hops:
            for call, counts in calls_of(B, hop).items():
                table[f"{name} hop {hop} {call}"] = record(lib, twin, mc, sd, B, hop, counts)
    return table


def write(table) -> None:
    """One line per launch."""
    with open(PATH, "w") as f:
        cases = [json.dumps(name) + ": [\n" + ",\n".join(" " + json.dumps(c, sort_keys=True) for c in table[name]) + "\n]" for name in sorted(table)]
        f.write("{\n" + ",\n".join(cases) + "\n}\n")


def main() -> None:
    import importlib
    import __graft_entry__ as ge
    ge.build()
    from quickvc_official_amd import lib as L
    write(collect(L.load_library(), ctypes.CDLL(importlib.import_module("quickvc_official_amd.build").build_emu_twin())))
    print(f"wrote {PATH} ({os.path.getsize(PATH) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
