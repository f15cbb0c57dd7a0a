"""Element-wise comparison of one launch's result against its host-emulated twin (tests/test_gpu_step_parity.py).

A snapshot is (workspace bytes, output fp32) after some step of a whole-path run.  Both sides of a comparison started
from the same snapshot, so every buffer the step did not write is bit-identical, and the ones it wrote may differ only
by fp32 accumulation order, transcendental implementations and rare one-ulp flips of a stored 2-byte value.  Errors
are counted per element over the VALID rows of every buffer (rows past a ragged member's end are never read unmasked,
so what a kernel leaves there is free): in ulps of the stored type for 2-byte buffers, relative to the buffer's RMS
for fp32 ones.
"""
import numpy as np
import torch

_TD = {"f16": torch.float16, "bf16": torch.bfloat16}


def output_spec(B, numel):
    """The path's output (waveform, or z for the posterior entry points) as one more fp32 'buffer', compared whole."""
    return dict(name="out", offset=0, bytes=numel * 4, elem="f32", groups=1, rows=numel // B, channels=1, mul=0, add=0)


def valid_rows(buf, lens, B):
    """[B] valid rows per member (see qvc_emu_workspace_map)."""
    rows = buf["rows"]
    if lens is None or buf["mul"] == 0:
        return [rows] * B
    return [max(0, min(rows, int(n) * buf["mul"] + buf["add"])) for n in lens]


def view(snap, buf, B):
    """(values float64 [G, B, rows, ch], ordered integers of the 2-byte patterns or None)."""
    ws, out = snap
    shape = (buf["groups"], B, buf["rows"], buf["channels"])
    if buf["name"] == "out":
        return out.double().reshape(shape), None
    raw = ws[buf["offset"]:buf["offset"] + buf["bytes"]]
    if buf["elem"] == "f32":
        return raw.view(torch.float32).double().reshape(shape), None
    bits = raw.view(torch.int16).reshape(shape).to(torch.int32)
    # sign-magnitude -> ordered: neighbouring representable values differ by 1 (+0 and -0 coincide)
    ordered = torch.where(bits < 0, -(bits & 0x7FFF), bits)
    return raw.view(_TD[buf["elem"]]).double().reshape(shape), ordered


def buffer_error(ref, got, buf, B, lens):
    """Per-element error of one buffer over its valid rows -> dict (None if every valid element is bit-identical).

    err: ulps of the stored type at max(|ref|, rms(ref)) (2-byte) or |got - ref| / rms(ref) (fp32); NaN / inf mismatches
    count as infinite."""
    rv, ro = view(ref, buf, B)
    gv, go = view(got, buf, B)
    mask = torch.zeros(buf["groups"], B, buf["rows"], 1, dtype=torch.bool)
    for b, n in enumerate(valid_rows(buf, lens, B)):
        mask[:, b, :n] = True
    mask = mask.expand_as(rv)
    if ro is not None:
        # ulps of the stored type at the element's magnitude, but never finer than at the buffer's RMS: a value near
        # zero that came out of a cancelling sum carries the absolute error of its terms, not of itself
        sel = rv[mask & torch.isfinite(rv)]
        rms = float(sel.pow(2).mean().sqrt()) if sel.numel() else 0.0
        mant = 10 if buf["elem"] == "f16" else 7
        mag = torch.clamp(torch.maximum(rv.abs(), torch.full_like(rv, rms)), min=2.0 ** -14)
        ulp = torch.exp2(torch.floor(torch.log2(mag)) - mant)
        err = torch.where(ro == go, torch.zeros_like(rv), (gv - rv).abs() / ulp)
        bad = (torch.isnan(rv) ^ torch.isnan(gv)) | (torch.isinf(rv) ^ torch.isinf(gv))
        err = torch.where(torch.isnan(rv) & torch.isnan(gv), torch.zeros_like(err), err)
        err = torch.where(torch.isfinite(err) | bad, err, torch.zeros_like(err))
    else:
        fin = torch.isfinite(rv) & torch.isfinite(gv)
        same = (rv == gv) | (torch.isnan(rv) & torch.isnan(gv))
        sel = rv[mask & torch.isfinite(rv)]
        rms = float(sel.pow(2).mean().sqrt()) if sel.numel() else 0.0
        err = torch.where(fin, (gv - rv).abs() / max(rms, 1e-30), torch.zeros_like(rv))
        bad = ~fin & ~same
    err = torch.where(bad, torch.full_like(err, float("inf")), err)
    err = torch.where(mask, err, torch.zeros_like(err))
    n_valid = int(mask.sum())
    n_diff = int((err > 0).sum())
    if n_diff == 0:
        return None
    flat = int(torch.argmax(err))
    g, b, t, c = np.unravel_index(flat, tuple(err.shape))
    return dict(buffer=buf["name"], elem=buf["elem"], max=float(err.reshape(-1)[flat]), n_diff=n_diff, n_valid=n_valid,
                frac=n_diff / max(n_valid, 1), n_over1=int((err > 1.0).sum()) if ro is not None else 0,
                where=dict(group=int(g), b=int(b), frame=int(t), frame_mod32=int(t) % 32, frame_mod64=int(t) % 64,
                           channel=int(c), channel_mod16=int(c) % 16),
                ref=float(rv[g, b, t, c]), got=float(gv[g, b, t, c]))


def compare_snapshots(ref, got, bufs, B, lens):
    """Every buffer (and the output) of two snapshots -> [buffer_error dicts of the buffers that differ]."""
    found = []
    for buf in bufs:
        e = buffer_error(ref, got, buf, B, lens)
        if e is not None:
            found.append(e)
    return found


def violations(found, kind, bounds, scratch=(), mode="f16"):
    """The entries of `found` that break the bounds of step kind `kind` (see BOUNDS; mode = the operand mode).  Buffers
    whose name starts with an entry of `scratch` (private scratch of that kind, read by no later step) are skipped."""
    lim = bounds[kind]
    rel = lim["rel_bf16"] if mode == "bf16" else lim["rel"]
    bad = []
    for e in found:
        if any(e["buffer"].startswith(p) for p in scratch):
            continue
        if e["elem"] == "f32":
            if not e["max"] <= rel:
                bad.append(e)
        elif not (e["max"] <= lim["ulp"] and e["n_over1"] <= lim["over1"] * e["n_valid"]):
            bad.append(e)
    return bad


def describe(e):
    w = e["where"]
    unit = "x RMS" if e["elem"] == "f32" else "ulp"
    return (f"{e['buffer']} ({e['elem']}): max error {e['max']:.3g} {unit} at group {w['group']} b {w['b']} frame {w['frame']} "
            f"(mod 32: {w['frame_mod32']}, mod 64: {w['frame_mod64']}) channel {w['channel']} (mod 16: {w['channel_mod16']}), "
            f"emulation {e['ref']:.6g} vs GPU {e['got']:.6g}; {e['n_diff']} of {e['n_valid']} valid elements differ, "
            f"{e['n_over1']} by more than one ulp")


# Bounds per step kind, set at most 4x over what the MI355X showed (profiles/r05_step_parity.txt):
#   ulp    max error of a stored 2-byte element, in ulps of its type at max(|value|, buffer RMS);
#   over1  max fraction of a buffer's valid elements more than one such ulp off;
#   rel    max fp32 error relative to the buffer's RMS (f16 and bf16x modes); rel_bf16 the same in the all-bf16 mode.
# frac_measured: the largest fraction of 2-byte elements seen to differ at all (the noise the comparator must accept).
# The separate sample launch is taken where proj keeps natural rows (the mini config at inter 256, plan info[0] == 0);
# its bounds are the conv epilogue's, which draws z the same way (profiles/r11_memory_contract.txt).
BOUNDS = {
    "gemv":      dict(ulp=0, over1=0.0, rel=2.5e-6, rel_bf16=2.5e-6),        # measured 6.3e-7
    "zero":      dict(ulp=0, over1=0.0, rel=0.0, rel_bf16=0.0),              # a memset: exact
    "conv":      dict(ulp=2, over1=1e-5, rel=2e-5, rel_bf16=2e-5),          # 1 ulp (0.15 % of elements); fp32 5.3e-6
    "sample":    dict(ulp=2, over1=1e-5, rel=2e-5, rel_bf16=2e-5),          # fp32 z 8.6e-7 (23 % of the elements differ at all)
    "wn":        dict(ulp=0, over1=0.0, rel=1.5e-3, rel_bf16=2.3e-2),       # fp32 3.8e-4 (f16; bf16 as wn_stack)
    "wn_stack":  dict(ulp=0, over1=0.0, rel=4.5e-3, rel_bf16=2.3e-2),       # fp32 1.1e-3 (f16, bf16x), 5.8e-3 (bf16)
    "pair3":     dict(ulp=4, over1=1.5e-4, rel=0.0, rel_bf16=0.0),          # 2 ulp (bf16x), 1 ulp (f16, bf16); 3.7e-5 over 1
    "chain":     dict(ulp=8, over1=1.5e-3, rel=0.0, rel_bf16=0.0),          # 3 ulp, 3.9e-4 over 1 (three pairs, f16)
    "post_tail": dict(ulp=0, over1=0.0, rel=1.6e-5, rel_bf16=1.6e-5),       # waveform 4.1e-6
    "tail":      dict(ulp=0, over1=0.0, rel=1.2e-5, rel_bf16=1.2e-5),       # waveform 2.9e-6
}
for _b in BOUNDS.values():
    _b["frac_measured"] = 0.021                                            # pair3, f16: 2.07 % of the stream, one ulp

# Private scratch: buffers the emulation writes in a step whose GPU kernel does not, and that no later step reads.
SCRATCH = {
    # rbchain_kernel keeps the ResBlock's stream on chip between its three pairs and writes only p[2].y (an `ra`
    # buffer); the emulation replays the chain pair by pair through p[0].y / p[1].y, so the `rb` buffer of a chained
    # ResBlock holds the emulation's middle tensor and the GPU's older bytes.  Nothing reads it afterwards.
    "chain": ("rb",),
}
