#!/usr/bin/env python3
"""Generates tests/golden/launch_trace.json: for every launch of a case, the CHOICE the chooser of its kernel family
returns (csrc/qvc_select.h: choose_conv, choose_pair, choose_chain, choose_wn, choose_wn_stack, choose_post_tail) -- the
kernel instantiation, the tile, the grid, the LDS size --, as the CPU twin's selecting backend records it
(tools/emu_twin.cpp: SelectBackend, qvc_emu_launch_trace).  tests/golden/path_trace.json pins what a launch is handed;
this file pins what the launcher then does with it.

Provenance: written on top of commit 7743cf2 ("One window driver: live_step and live_tick share live_run and one state"),
in this order: the selection rules of that commit's device headers (choose_tile, choose_pair_tile, the chunk-loop test,
the blocks32 rule, the tiny-batch rule, wn_stack_variant, the post_tail_nf switch, chain_pick_nf, wn2_supported and the
argument checks in front of them) were moved verbatim into csrc/qvc_select.h; the file was generated from them; only then
were the dispatchers of the device translation units rewritten to consume a choice.  tests/test_launch_trace_host.py
asserts that the present choosers give exactly these choices.  The file is never regenerated: a change that is meant to
move a choice edits it (--dump shows what a case records now) and says why.

Per case {"names": the calls in order, "hashes": a 16-hex-digit hash of each call's words}.  A launch-family call's words
are the inputs the rules read, every field of its LaunchChoice and whether the chosen tuple is instantiated; the other
calls have none (tail: its bands).  Needs no GPU.

    python tests/golden/make_golden_launch_trace.py [--dump CASE]
"""
from __future__ import annotations

import ctypes
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _path_trace():
    spec = importlib.util.spec_from_file_location("make_golden_path_trace", os.path.join(HERE, "make_golden_path_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


PT = _path_trace()
PATH = os.path.join(HERE, "launch_trace.json")
FAMILIES = ("conv", "pair", "chain", "wn_layer", "wn_stack", "wn_stack2", "post_tail")     # csrc/qvc_select.h: LaunchFamily
FAMILY_KINDS = ("conv", "pair3", "chain", "wn", "wn_stack", "post_tail")                  # the calls that carry a choice
EPI_STD = 0
LDS_MAX = 160 * 1024
# the export's order: the five switches of the path trace, then the three the choosers read; the defaults
SWITCHES = dict(PT.SWITCHES, conv_cl=1, post_tail_nf=4, wn_kernel=0)
# The shipped model at sizes on both sides of every threshold (B, T): one utterance; the chunk-loop and up-sampler rules
# below their 512 workgroups; a full chip (256 32-frame WaveNet tiles); 512 of them (the per-layer kernel's 64-frame tile).
SHIPPED_SHAPES = ((1, 64), (4, 96), (32, 256), (32, 512))
STREAM_SHAPES = ((4, 24), (32, 96))
# the selection-relevant switches at each non-default value, at a small and a chip-filling shape
SELECT_SWITCHES = (("conv_cl", 0), ("post_tail_nf", 2), ("wn_kernel", 1), ("wn_kernel", 2), ("wn_kernel", 3), ("pair_chain3", 1))
SWITCH_SHAPES = ((1, 64), (32, 256))


def cases():
    """{case name: (model, form, B, T, U, switches)}: every case of the path trace, then the shipped model's own."""
    table, all_models = PT.cases()
    out = {case: (model, form, B, T, U, dict(SWITCHES, **sw)) for case, (model, form, B, T, U, sw) in table.items()}

    def add(form, B, T, **sw):
        tag = "".join(" %s=%d" % kv for kv in sw.items())
        out[f"shipped {form} B{B} T{T}{tag}"] = ("shipped", PT.FORMS.index(form), B, T, 1, dict(SWITCHES, **sw))
    for B, T in SHIPPED_SHAPES:
        add("uniform", B, T)
    for B, T in STREAM_SHAPES:
        add("stream_dec", B, T)
    for name, value in SELECT_SWITCHES:
        for B, T in SWITCH_SHAPES:
            add("uniform", B, T, **{name: value})
    add("uniform", 32, 512, wn_chunk=-1)      # one launch per WaveNet layer, 512 32-frame tiles
    return out, all_models


def declare(twin):
    from quickvc_official_amd import lib as L
    I, Lg = ctypes.c_int32, ctypes.c_int64
    twin.qvc_emu_launch_trace.restype = ctypes.c_int
    twin.qvc_emu_launch_trace.argtypes = [ctypes.POINTER(L.QvcConfig), I, I, I, I, ctypes.POINTER(I), ctypes.POINTER(Lg), Lg, ctypes.POINTER(Lg)]
    twin.qvc_emu_launch_trace_layout.restype = Lg
    twin.qvc_emu_launch_trace_layout.argtypes = [ctypes.c_char_p, Lg]
    return twin


def layout(twin):
    """{kind: [name of every word]} and the kinds in the order of their index (tools/emu_twin.cpp: kTraceKinds)."""
    n = twin.qvc_emu_launch_trace_layout(None, 0)
    text = ctypes.create_string_buffer(n)
    assert twin.qvc_emu_launch_trace_layout(text, n) == n
    lines = [line.split(" ") for line in text.value.decode().splitlines()]
    return {line[0]: line[1:] for line in lines}, [line[0] for line in lines]


def record(twin, kinds, mc, form, B, T, U, switches, dtype="f16"):
    """[(kind, [words])] of one call of qvc_emu_launch_trace."""
    from quickvc_official_amd import lib as L
    cfg = L.make_config(dict(mc, operand_dtype=dtype))
    sw = (ctypes.c_int32 * len(SWITCHES))(*[switches[k] for k in SWITCHES])
    cap = 1 << 18
    rec, used = (ctypes.c_int64 * cap)(), ctypes.c_int64(0)
    st = twin.qvc_emu_launch_trace(ctypes.byref(cfg), form, B, T, U, sw, rec, cap, ctypes.byref(used))
    assert st == 0, ("qvc_emu_launch_trace", PT.FORMS[form], st)
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


def compress(full):
    return {case: {"names": " ".join(k for k, _ in recs), "hashes": " ".join(PT.digest(w) for _, w in recs)} for case, recs in full.items()}


def collect(twin):
    """The table in the golden file's form."""
    return compress(collect_full(twin)[0])


def choices(full, names):
    """[(case, kind, {word name: value})] of every launch-family call."""
    return [(case, kind, dict(zip(names[kind], w))) for case, rs in full.items() for kind, w in rs if kind in FAMILY_KINDS]


DTYPE_NAMES = {0: "bf16", 1: "f16", 2: "bf16x"}      # include/qvc.h: QVC_BF16, QVC_F16, QVC_BF16X


def record_names(recs, names):
    """The record names qvc_infer_batch_timed gives the launches of one traced call (csrc/qvc_api.hip: TimedBackend names its
    records from the same choices): one per launch; fork / join and the closing "steps" record are no launches."""
    out = []
    for kind, w in recs:
        r = dict(zip(names.get(kind, ()), w))
        tn = DTYPE_NAMES.get(r.get("dtype"))
        if kind == "conv":
            out.append("conv<%s,MF%d,NF%d,WM%d,%s>" % (tn, r["c.MF"], r["c.NF"], r["c.WM"], {1: "gau", 3: "smp"}.get(r["epi"], "std")))
        elif kind == "pair3":
            out.append("rbpair<%s,MF%d,NF%d,WM%d>" % (tn, r["c.MF"], r["c.NF"], r["c.WM"]))
        elif kind == "chain":
            out.append("rbchain<%s,MF%d,NF%d,WM%d,k%d>" % (tn, r["c.MF"], r["c.NF"], r["c.WM"], r["k"]))
        elif kind == "wn":
            out.append("wn_layer<%s,W%d,NF%d%s>" % (tn, r["W"], r["c.NF"], ",last" if r["c.last"] else ""))
        elif kind == "wn_stack":
            stream = r["c.family"] == FAMILIES.index("wn_stack2")
            out.append("%s<%s,W%d,L%d%s%s>" % ("wn_stack2" if stream else "wn_stack", tn, r["W"], r["layers"], ",pre+post" if r["fused"] else "",
                                               ",64f" if stream and r["c.NF"] == 5 else ""))
        elif kind == "post_tail":
            out.append(("post_tail1<%s>" if r["c.bands"] == 1 else "post_tail<%s>") % tn)
        elif kind == "tail":
            out.append("istft1" if r["bands"] == 1 else "istft_synth")
        elif kind in ("gemv", "sample", "zero"):
            out.append({"gemv": "cond_gemv", "sample": "sample", "zero": "memset"}[kind])
        else:
            assert kind in ("fork", "branch", "branch_done", "join", "steps"), kind
    return out


def check_choices(full, names):
    """Every choice is a launch the library can make: accepted, an instantiated tuple, within the LDS of a CU."""
    for case, kind, r in choices(full, names):
        assert len(r) == len(names[kind]), (case, kind, "layout")
        assert r["c.status"] == 0, (case, kind, r)
        assert r["built"] == 1, (case, kind, r)
        assert 0 <= r["c.lds"] <= LDS_MAX, (case, kind, r)


def check_coverage(full, names):
    """Every rule of the choosers fires in both directions somewhere in the table (asserted before the file is written):
    a rule seen on one side only is a rule the file does not pin."""
    recs = choices(full, names)
    fam = FAMILIES.index

    def cdiv(a, b):
        return -(-a // b)

    def default(case, *switch):     # the case runs with these switches at their defaults
        return not any(f" {s}=" in case for s in switch)

    def both(what, fired, kept):
        assert fired, f"{what}: never fires"
        assert kept, f"{what}: fires in every case"
    conv = [(c, r) for c, k, r in recs if k == "conv"]
    # the conv early return: at the smallest tile (NF 2) every workgroup has a CU of its own (blocks <= 256)
    blocks2 = lambda r: cdiv(r["Nq"], (4 // r["c.WM"]) * 32) * r["batch"] * r["nchunk"]
    both("conv early return", [r for _c, r in conv if blocks2(r) <= 256 and r["c.NF"] == 2], [r for _c, r in conv if blocks2(r) > 256])
    # the up-sampler rule: NF < 4 is skipped from 512 workgroups of 64-frame tiles on
    ups = lambda r: cdiv(r["Nq"], (4 // r["c.WM"]) * 64) * r["batch"] * r["nchunk"]
    both("up-sampler 512-block rule", [r for _c, r in conv if r["up_s"] > 1 and ups(r) >= 512 and r["c.NF"] >= 4],
         [r for _c, r in conv if r["up_s"] > 1 and ups(r) < 512])
    # the chunk loop, among the launches it is built for
    cl_ok = [(c, r) for c, r in conv if r["c.epi"] == EPI_STD and r["c.MF"] == 4 and r["c.WM"] == 4 and r["c.NF"] <= 5 and r["nchunk"] >= 2 and r["mean3"]]
    tiles = lambda r: r["c.grid[0]"] * r["batch"]
    both("chunk loop", [r for c, r in cl_ok if default(c, "conv_cl") and r["c.cl"] == 1 and tiles(r) >= 512],
         [r for c, r in cl_ok if default(c, "conv_cl") and r["c.cl"] == 0 and tiles(r) < 512])
    assert [r for c, r in cl_ok if " conv_cl=0" in c and r["c.cl"] == 0 and tiles(r) >= 512], "conv_cl = 0"
    # the WaveNet layer's 64-frame tile from 512 32-frame workgroups on
    wn = [r for _c, k, r in recs if k == "wn"]
    both("wn_layer blocks32 >= 512", [r for r in wn if r["c.NF"] == 4 and cdiv(r["T"], 32) * r["batch"] >= 512],
         [r for r in wn if r["c.NF"] == 2 and cdiv(r["T"], 32) * r["batch"] < 512])
    st = [(c, r, cdiv(r["T"], 32) * r["batch"]) for c, k, r in recs if k == "wn_stack"]
    # the wide tile of the continuous-stream kernel: where the caller allows it and the 32-frame grid fills the chip
    st2 = [(c, r, t) for c, r, t in st if r["c.family"] == fam("wn_stack2") and default(c, "wn_kernel")]
    both("wide WaveNet tile", [r for _c, r, t in st2 if r["wide"] == 1 and t >= 256 and r["c.NF"] == 5],
         [r for _c, r, t in st2 if r["wide"] == 1 and t < 256 and r["c.NF"] == 3])
    # the 16-frame tile of the generic stack kernel up to 64 32-frame tiles
    gen = [(r, t) for _c, r, t in st if r["c.family"] == fam("wn_stack")]
    both("16-frame stack tile", [r for r, t in gen if r["c.NF"] == 2 and t <= 64], [r for r, t in gen if r["c.NF"] == 3 and t > 64])
    assert [r for r, _t in gen if r["c.NF"] == 6], "the six-fragment window of the generic stack kernel"
    pair = [r for _c, k, r in recs if k == "pair3"]
    both("pair layouts", [r for r in pair if r["c.waves"] == 8], [r for r in pair if r["c.waves"] == 4])
    post = [(c, r) for c, k, r in recs if k == "post_tail"]
    both("post_tail bands", [r for _c, r in post if r["c.bands"] == 1], [r for _c, r in post if r["c.bands"] == 4 and r["c.NF"] == 4])
    # the switches at their non-default values
    assert [r for c, r in post if " post_tail_nf=2" in c and r["c.bands"] == 4 and r["c.NF"] == 2], "post_tail_nf = 2"
    for value, family, nf in ((1, "wn_stack", (2, 3)), (2, "wn_stack2", (3,)), (3, "wn_stack2", (5,))):
        for B, T in SWITCH_SHAPES:
            got = {(r["c.family"], r["c.NF"]) for c, r, _t in st if c == f"shipped uniform B{B} T{T} wn_kernel={value}"}
            assert got and got <= {(fam(family), n) for n in nf}, ("wn_kernel", value, B, T, got)
    assert [r for c, k, r in recs if k == "chain" and " pair_chain3=1" in c], "pair_chain3 = 1"
    assert {r["c.family"] for _c, _k, r in recs} == set(range(len(FAMILIES))), "a kernel family without a launch"


def write(table) -> None:
    """One line per case."""
    with open(PATH, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(name) + ": " + json.dumps(table[name], sort_keys=True) for name in sorted(table)) + "\n}\n")


def dump(full, names, case) -> None:
    for i, (kind, words) in enumerate(full[case]):
        print(f"{i:4d} {kind} {PT.digest(words)}: " + " ".join(f"{n}={v}" for n, v in zip(names.get(kind, ()), words)))


def main() -> None:
    import importlib
    twin = ctypes.CDLL(importlib.import_module("quickvc_official_amd.build").build_emu_twin())
    full, names = collect_full(twin)
    if "--dump" in sys.argv:
        return dump(full, names, sys.argv[sys.argv.index("--dump") + 1])
    check_choices(full, names)
    check_coverage(full, names)
    write(compress(full))
    print(f"wrote {PATH} ({os.path.getsize(PATH) / 1024:.0f} KiB, {len(full)} cases, {sum(len(r) for r in full.values())} records)")


if __name__ == "__main__":
    main()
