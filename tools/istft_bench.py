#!/usr/bin/env python3
"""Developer benchmark of the single-band iSTFT decoder (ISTFT_MODEL_CONFIG, istft_vits=True): B x T unit frames
per step (default 32 x 250 = 32 utterances of 5 s), f16 and bf16x, warmed up, timed with device events.

    python tools/istft_bench.py [--batch 32 --frames 250 --steps 20 --warmup 5]
        -> one JSON line per operand mode: ms/step, samples/s, RTF, SNR of the timed outputs against the test-side
           restatement (tests/istft_ref.py, fp32 on the CPU, first --snr-utts utterances)
    python tools/istft_bench.py --steps 3 --warmup 1 --no-snr      (run under rocprofv3 --kernel-trace --stats)
    python tools/istft_bench.py --tail-stats <kernel_stats.csv> [--batch 32 --frames 250]
        -> the fused single-band tail's mean kernel time from that profile, as achieved bytes/s over its algorithmic
           bytes (three stage-final ResBlock streams read once + the waveform written once) and as a fraction of
           6.29 TB/s (the measured HBM copy rate)
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_COPY = 6.29e12


def tail_bytes(cfg, batch, frames):
    """Algorithmic bytes of post_tail_kernel<T, 2, 1>: three f16 streams of the last stage in, fp32 waveform out."""
    t, ch = frames, cfg["upsample_initial_channel"]
    for _u in cfg["upsample_rates"]:
        t *= _u
        ch //= 2
    return batch * (t * ch * 2 * 3 + 4 * t * 4)


def tail_stats(path, cfg, batch, frames):
    rows = list(csv.DictReader(open(path)))
    hits = [r for r in rows if "post_tail_kernel" in r.get("Name", r.get("KernelName", ""))]
    if not hits:
        raise SystemExit(f"no post_tail_kernel row in {path}")
    r = hits[0]
    ns = float(r.get("AverageNs") or r.get("AverageDurationNs") or float(r["TotalDurationNs"]) / float(r["Calls"]))
    by = tail_bytes(cfg, batch, frames)
    return {"kernel": r.get("Name", r.get("KernelName")), "calls": int(r["Calls"]), "mean_us": ns / 1e3,
            "algorithmic_MB": by / 1e6, "achieved_TBps": by / (ns * 1e-9) / 1e12, "fraction_of_6.29TBps": by / (ns * 1e-9) / HBM_COPY}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtypes", default="bf16x,f16")
    ap.add_argument("--snr-utts", type=int, default=2)
    ap.add_argument("--no-snr", action="store_true")
    ap.add_argument("--tail-stats", default=None)
    args = ap.parse_args()
    import quickvc_official_amd as q
    cfg = q.ISTFT_MODEL_CONFIG
    if args.tail_stats:
        print(json.dumps(tail_stats(args.tail_stats, cfg, args.batch, args.frames)))
        return
    import torch
    from quickvc_official_amd.engine import QvcEngine
    from quickvc_official_amd.synth import make_synthetic_state_dict, make_synthetic_inputs
    dev = torch.device("cuda:0")
    model = q.SynthesizerTrn(641, 32, **cfg)
    sd = make_synthetic_state_dict(model, 1234)
    B, T = args.batch, args.frames
    unit, g, noise = make_synthetic_inputs(B, T, 256, cfg["inter_channels"], cfg["gin_channels"], seed0=0)
    ud, gd, nd = unit.to(dev), g.to(dev), noise.to(dev)
    ref = None
    for dt in args.dtypes.split(","):
        eng = QvcEngine(dict(model.model_config, operand_dtype=dt), sd, dev)
        out = torch.empty(B, 1, T * eng.samples_per_frame, device=dev)
        for _ in range(args.warmup):
            eng.infer_batch(ud, gd, nd, out=out)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        ev[0].record()
        for i in range(args.steps):
            eng.infer_batch(ud, gd, nd, out=out)
            ev[i + 1].record()
        torch.cuda.synchronize()
        ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps))
        med = ms[len(ms) // 2]
        samples = B * T * eng.samples_per_frame
        res = {"config": "ISTFT_MODEL_CONFIG", "dtype": dt, "batch": B, "frames": T, "steps": args.steps,
               "ms_per_step_median": med, "ms_per_step_min": ms[0], "samples_per_s": samples / (med * 1e-3),
               "rtf": (med * 1e-3) / (samples / 16000.0)}
        if not args.no_snr:
            import istft_ref
            from helpers import snr_db
            n = min(args.snr_utts, B)
            if ref is None:
                t0 = time.time()
                ref = istft_ref.infer_from_g_single(sd, cfg, unit[:n], g[:n].unsqueeze(-1), noise[:n])
                res["restatement_s"] = time.time() - t0
            got = out[:n].cpu()
            res["snr_db_vs_restatement"] = [snr_db(ref[b], got[b]) for b in range(n)]
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
