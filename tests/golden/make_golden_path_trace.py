#!/usr/bin/env python3
"""Generates tests/golden/path_trace.json: every backend call of csrc/qvc_path.h -- the launches the GPU is handed and the
fork / join around the unfused stages --, as the CPU twin's recording backend sees them (tools/emu_twin.cpp: TraceBackend,
qvc_emu_path_trace).

The file pins the WORK of the path, not its values: it was written at commit 7c06bfe ("One segment-ring body: stream_step
and stream_tick share stream_run"), the last one in which Path::dec_part was one function, with the twin built against that
commit's csrc/qvc_path.h and csrc/qvc_api.hip (only wn_chunk() had moved, verbatim, into csrc/qvc_kernels.h, so that the
recording backend answers wn_stack_chunk as HipBackend does).  tests/test_path_trace_host.py asserts that the present
Path issues exactly these calls.  The file is never regenerated: a change that is meant to move a launch, or a field of one,
edits it (--dump shows what a case records now) and says why.

Per case {"names": the calls in order, "hashes": a 16-hex-digit hash of each call's words}.  A call's words are its
non-Args parameters, the ConvDesc fields the launchers read and every field of its Args struct, pointers as (region, byte
offset) with the regions of REGIONS; a Path form ends with a "steps" record, the StepKind of every step.  The records do
not depend on data -- Path never reads a device pointer -- so the buffers are sized and never filled.  Needs no GPU.

    python tests/golden/make_golden_path_trace.py [--dump CASE]
"""
from __future__ import annotations

import ctypes
import hashlib
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PATH = os.path.join(HERE, "path_trace.json")
REGIONS = ("blob", "workspace", "unit", "g", "noise", "out", "lens", "pos", "frames", "src", "row_frames", "keys", "mel", "z/spec", "state", "null")
FORMS = ("uniform", "ragged_fm", "ragged_rng", "fanout", "fanout_rng", "enc_q", "flow_forward", "enc_p", "dec_trunk", "stream_dec", "spk", "spk_ragged")
STEP_KINDS = ("conv", "zero", "gemv", "sample", "wn", "wn_stack", "chain", "pair3", "post_tail", "post_tail1", "tail", "tail1", "sample_rows")
EPI_SAMPLE, EPI_STATS = 3, 4
SWITCHES = {"pair_chain3": 0, "post_tail": 1, "wn_chunk": 0, "pair_cm4": 1, "pair_wide_launch": 1}     # the export's order, the defaults
NON_DEFAULT = (("pair_chain3", 1), ("wn_chunk", -1), ("wn_chunk", 2), ("post_tail", 0), ("pair_cm4", 0), ("pair_wide_launch", 0))
SMALL = (2, 23)                     # tests/config_space.py: B, T
BIG_ROWS = ("shipped", "mb_up16_up1", "istft_ups3", "one_up8_init528")     # the shipped model, multiband, single band, unfused pairs
BIG_B, FAN_SOURCES, SPK_UTTERANCES, SPK_FRAMES = 3, 2, 2, 200            # 200 mel frames: three partials per utterance


def models():
    """{name: model_config}: every row of tests/config_space.py, the shipped configuration and MINI_MODEL_CONFIG."""
    import quickvc_official_amd as q
    import config_space as CS
    out = {}
    for name, row in CS.ROWS.items():
        cfg = CS.constructor_config(name)
        mc = dict(q.SynthesizerTrn(641, 32, **cfg).model_config)
        if row["wn"] is not None:
            mc.update({key: cfg[key] for key in ("wn_kernel_size", "enc_layers", "flow_layers", "n_flows")})
        out[name] = mc
    out["shipped"] = dict(q.SynthesizerTrn(641, 32, **q.DEFAULT_MODEL_CONFIG).model_config)
    out["MINI_MODEL_CONFIG"] = dict(q.SynthesizerTrn(641, 32, **q.MINI_MODEL_CONFIG).model_config)
    return out


def big_frames(mc, B):
    """The smallest T at which no stage of the plan has few_tiles (csrc/qvc_path.h: B * t_out * n_resblocks <= 256 * 32),
    made odd: a multiple of no tile size."""
    nb, rate, T = len(mc["resblock_kernel_sizes"]), 1, 0
    for s in mc["upsample_rates"]:
        rate *= s
        T = max(T, 256 * 32 // (B * rate * nb) + 1)
    T |= 1
    rate = 1
    for s in mc["upsample_rates"]:
        rate *= s
        assert B * T * rate * nb > 256 * 32, (mc["upsample_rates"], B, T)
    return T


def cases():
    """{case name: (model, form, B, T, U, switches)}."""
    out = {}

    def add(model, form, B, T, U=1, **sw):
        tag = "".join(" %s=%d" % kv for kv in sw.items())
        out[f"{model} {form} B{B} T{T}{tag}"] = (model, FORMS.index(form), B, T, U, dict(SWITCHES, **sw))
    all_models = models()
    for model in all_models:
        for form in ("uniform", "ragged_fm"):
            add(model, form, *SMALL)
    for model in BIG_ROWS:
        T = big_frames(all_models[model], BIG_B)
        for form in FORMS:
            if form.startswith("spk"):
                add(model, form, 1, SPK_FRAMES, SPK_UTTERANCES)
            else:
                add(model, form, BIG_B, T, FAN_SOURCES if form.startswith("fanout") else 1)
        for name, value in NON_DEFAULT:
            add(model, "uniform", BIG_B, T, **{name: value})
    return out, all_models


def declare(twin):
    from quickvc_official_amd import lib as L
    I, Lg = ctypes.c_int32, ctypes.c_int64
    twin.qvc_emu_path_trace.restype = ctypes.c_int
    twin.qvc_emu_path_trace.argtypes = [ctypes.POINTER(L.QvcConfig), I, I, I, I, ctypes.POINTER(I), ctypes.POINTER(Lg), Lg, ctypes.POINTER(Lg)]
    twin.qvc_emu_path_trace_layout.restype = Lg
    twin.qvc_emu_path_trace_layout.argtypes = [ctypes.c_char_p, Lg]
    return twin


def layout(twin):
    """{kind: [name of every word]} and the kinds in the order of their index (tools/emu_twin.cpp: kTraceKinds)."""
    n = twin.qvc_emu_path_trace_layout(None, 0)
    text = ctypes.create_string_buffer(n)
    assert twin.qvc_emu_path_trace_layout(text, n) == n
    lines = [line.split(" ") for line in text.value.decode().splitlines()]
    return {line[0]: line[1:] for line in lines}, [line[0] for line in lines]


def record(twin, kinds, mc, form, B, T, U, switches):
    """[(kind, [words])] of one call of qvc_emu_path_trace."""
    from quickvc_official_amd import lib as L
    cfg = L.make_config(dict(mc, operand_dtype="f16"))
    sw = (ctypes.c_int32 * len(SWITCHES))(*[switches[k] for k in SWITCHES])
    cap = 1 << 20
    rec, used = (ctypes.c_int64 * cap)(), ctypes.c_int64(0)
    st = twin.qvc_emu_path_trace(ctypes.byref(cfg), form, B, T, U, sw, rec, cap, ctypes.byref(used))
    assert st == 0, ("qvc_emu_path_trace", FORMS[form], st)
    words, out, i = rec[:used.value], [], 0
    while i < len(words):
        kind, n = kinds[words[i]], words[i + 1]
        out.append((kind, words[i + 2:i + 2 + n]))
        i += 2 + n
    return out


def collect_full(twin):
    """{case: [(kind, [words])]} from the CPU twin `twin`, and the layout of the records."""
    declare(twin)
    names, kinds = layout(twin)
    table, all_models = cases()
    return {case: record(twin, kinds, all_models[model], *rest) for case, (model, *rest) in table.items()}, names


def digest(words):
    return hashlib.blake2b(struct.pack("<%dq" % len(words), *words), digest_size=8).hexdigest()


def compress(full):
    return {case: {"names": " ".join(k for k, _ in recs), "hashes": " ".join(digest(w) for _, w in recs)} for case, recs in full.items()}


def collect(twin):
    """The table in the golden file's form."""
    return compress(collect_full(twin)[0])


def check_coverage(full, names):
    """What the table must hold (asserted over all cases before the file is written)."""
    null, state = REGIONS.index("null"), REGIONS.index("state")
    recs = [(case, kind, dict(zip(names[kind], w))) for case, rs in full.items() for kind, w in rs if kind != "steps"]
    for case, kind, r in recs:
        assert len(r) == len(names[kind]), (case, kind, "layout")

    def some(kind, pred):
        return any(k == kind and pred(r) for _c, k, r in recs)
    steps = {s for rs in full.values() for kind, w in rs if kind == "steps" for s in w}
    assert steps == set(range(len(STEP_KINDS))), sorted(STEP_KINDS[s] for s in set(range(len(STEP_KINDS))) - steps)
    assert some("pair3", lambda r: r["n"] == 3 and r["chain_major"] == 1)
    assert some("pair3", lambda r: r["n"] == 3 and r["chain_major"] == 0)
    assert some("pair3", lambda r: r["n"] == 1)
    assert any(" fork branch conv conv " in " " + " ".join(k for k, _ in rs) and " join " in " ".join(k for k, _ in rs) + " " for rs in full.values())
    assert some("wn_stack", lambda r: r["w_pre"] != null) and some("wn_stack", lambda r: r["w_pre"] == null)
    assert some("wn_stack", lambda r: r["accum"] == 1) and some("wn_stack", lambda r: r["final_layer"] == 0)
    assert some("conv", lambda r: r["epi"] == EPI_SAMPLE and r["a.rng.keys"] != null)
    assert some("conv", lambda r: r["epi"] == EPI_SAMPLE and r["a.rng.keys"] == null)
    assert some("conv", lambda r: r["epi"] == EPI_STATS)
    assert some("post_tail", lambda r: r["fir"] != null) and some("post_tail", lambda r: r["fir"] == null)
    assert some("tail", lambda r: r["bands"] == 1)
    # a dec_back_wave whose mean_input reads s0_override: the streaming form's consumer of stage 0 stages the hand-over
    assert any("stream_dec" in c and ((k == "conv" and r["a.x"] == state and r["a.x3"] == state) or (k == "post_tail" and r["c.x"] == state))
               for c, k, r in recs)


def write(table) -> None:
    """One line per case."""
    with open(PATH, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(name) + ": " + json.dumps(table[name], sort_keys=True) for name in sorted(table)) + "\n}\n")


def dump(full, names, case) -> None:
    for i, (kind, words) in enumerate(full[case]):
        fields = zip(names[kind], words) if kind != "steps" else ((str(s), STEP_KINDS[k]) for s, k in enumerate(words))
        print(f"{i:4d} {kind} {digest(words)}: " + " ".join(f"{n}={v}" for n, v in fields))


def main() -> None:
    import importlib
    import __graft_entry__ as ge
    ge.build()
    twin = ctypes.CDLL(importlib.import_module("quickvc_official_amd.build").build_emu_twin())
    full, names = collect_full(twin)
    if "--dump" in sys.argv:
        return dump(full, names, sys.argv[sys.argv.index("--dump") + 1])
    check_coverage(full, names)
    write(compress(full))
    print(f"wrote {PATH} ({os.path.getsize(PATH) / 1024:.0f} KiB, {len(full)} cases, {sum(len(r) for r in full.values())} records)")


if __name__ == "__main__":
    main()
