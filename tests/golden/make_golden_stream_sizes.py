#!/usr/bin/env python3
"""Generates tests/golden/stream_sizes.json: what the three streaming forms (qvc_stream_*, qvc_live_*, qvc_live_tick_*)
report for their buffers, and where the tick twin places every slot's rings.

The file pins the ring geometry of csrc/qvc_stream.h byte for byte: it was written at the commit BEFORE the rings were
stated once in a table, and tests/test_stream_sizes_host.py asserts that the library still returns exactly these values.
Regenerate it only when a ring is meant to change.

Per config (the three shipped ones and five rows of tests/config_space.py): lag, noise lag and context frames; per
(B, hop) the segment-ring state / workspace bytes; per (B, hop, L), L in {0, 4, context}, the state / workspace bytes of
the windowed step and of its tick form, and (offset, bytes) of every slot's unit and noise ring as the CPU twin reports
them.  A refusal is recorded as its (negative) status code.  Needs no GPU.

    python tests/golden/make_golden_stream_sizes.py
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

SHIPPED = ("DEFAULT_MODEL_CONFIG", "MINI_MODEL_CONFIG", "ISTFT_MODEL_CONFIG")
ROWS = ("one_up8", "mb_up16_up1", "istft_ups3", "istft_ups4", "rb_k1_k15_k13")
BATCHES, HOPS = (1, 3), (1, 7, 16)
PATH = os.path.join(HERE, "stream_sizes.json")


def configs():
    """{name: qvc_config} of the shipped model configs and the rows of the configuration space."""
    import config_space as CS
    import quickvc_official_amd as q
    from quickvc_official_amd import lib as L
    out = {name: L.make_config(q.SynthesizerTrn(641, 32, **getattr(q, name)).model_config) for name in SHIPPED}
    out.update({row: L.make_config(CS.problem(row)[1]) for row in ROWS})
    return out


def collect(lib, twin):
    """The table, from the product library `lib` and the CPU twin `twin` (qvc_emu_live_tick_ring declared)."""
    table = {}
    for name, cfg in configs().items():
        p = ctypes.byref(cfg)
        context = int(lib.qvc_live_context_frames(p))
        row = {"lag": int(lib.qvc_stream_lag_frames(p)), "noise_lag": int(lib.qvc_stream_noise_lag_frames(p)), "context": context,
               "stream": {}, "live": {}, "tick": {}, "tick_rings": {}}
        for B in BATCHES:
            for hop in HOPS:
                row["stream"][f"{B},{hop}"] = [int(lib.qvc_stream_state_bytes(p, B, hop)), int(lib.qvc_stream_workspace_bytes(p, B, hop))]
                for look in (0, 4, context):
                    key = f"{B},{hop},{look}"
                    row["live"][key] = [int(lib.qvc_live_state_bytes(p, B, hop, look)), int(lib.qvc_live_workspace_bytes(p, B, hop, look))]
                    row["tick"][key] = [int(lib.qvc_live_tick_state_bytes(p, B, hop, look)), int(lib.qvc_live_tick_workspace_bytes(p, B, hop, look))]
                    if row["tick"][key][0] < 0:
                        continue
                    rings = []
                    for slot in range(B):
                        for which in (0, 1):
                            off, n = ctypes.c_int64(-1), ctypes.c_int64(-1)
                            st = twin.qvc_emu_live_tick_ring(p, B, hop, look, slot, which, ctypes.byref(off), ctypes.byref(n))
                            rings.append([int(off.value), int(n.value)] if st == 0 else int(st))
                    row["tick_rings"][key] = rings
        table[name] = row
    return table


def load_twin():
    import importlib
    from quickvc_official_amd import lib as L
    twin = ctypes.CDLL(importlib.import_module("quickvc_official_amd.build").build_emu_twin())
    I, Lg = ctypes.c_int32, ctypes.c_int64
    twin.qvc_emu_live_tick_ring.restype = ctypes.c_int
    twin.qvc_emu_live_tick_ring.argtypes = [ctypes.POINTER(L.QvcConfig), I, I, I, I, I, ctypes.POINTER(Lg), ctypes.POINTER(Lg)]
    return twin


def write(table) -> None:
    """One line per config."""
    with open(PATH, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(name)}: {json.dumps(table[name], sort_keys=True)}" for name in sorted(table)) + "\n}\n")


def main() -> None:
    import __graft_entry__ as ge
    ge.build()
    from quickvc_official_amd import lib as L
    write(collect(L.load_library(), load_twin()))
    print(f"wrote {PATH} ({os.path.getsize(PATH) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
