#!/usr/bin/env python3
"""bench.py -- headline benchmark of the QuickVC hot path on MI355X (BASELINE.json).

Metric: audio samples/s (+ RTF) for offline voice conversion of 16 kHz 5 s utterances,
batch 32 per GPU (BASELINE.json configs[2]; weak scaling: every rank converts its own
batch, no per-step collective -- the only collective is one weight broadcast at start-up).

One "step" = one pass of the whole hot path (enc_p -> reverse flow -> generator -> iSTFT +
band synthesis) over one batch of 32 synthetic utterances already resident in HBM.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
                                                                  (N > 1: starts its own N worker processes, one per GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times the K steps, writes the last step's output if --dump-outputs is given, and
rank 0 prints ONE JSON line (metric, value, unit, higher_is_better, dtype, ms_per_step, ...).
With --full the line also holds the legs that take runs of their own:
  "steady_state" / "one_batch_at_a_time": the K steps timed again at the steady clock, and on one lane only;
  "roofline":     the dominant kernel's achieved TFLOP/s vs the gfx950 dense f16/bf16 MFMA peak,
                  from per-launch HIP events (qvc_infer_batch_timed) on the launch stream;
  "speaker_encoder": the time of one speaker-embedding call for the batch;
  "cpu_baseline" / "parity": the fp32 CPU oracle (a port of the reference path) timed on this host's
                  cores on a bounded sample of the same workload, and the GPU output against it (N=1 only).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SAMPLE_RATE = 16000
FRAMES = 250            # 5 s of 320-sample unit frames
BATCH = 32
PEAK_MFMA_TFLOPS = 2500.0      # dense bf16/f16 MFMA, MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0


def kernel_source_sha1() -> str:
    """Hash of the kernel sources: ties a PMC traffic file to the code it was measured on (no git on the GPU box)."""
    import hashlib
    h = hashlib.sha1()
    csrc = os.path.join(ROOT, "quickvc-official_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".h", ".hip", ".cpp")):
            h.update(open(os.path.join(csrc, name), "rb").read())
    return h.hexdigest()


def launch_workers(n: int, argv, rehearsal: bool) -> int:
    """--gpus N without a launcher: start N fresh worker processes (one rank per GPU, RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_* as torch.distributed.run would set them) BEFORE this process touches the GPU, forward rank 0's JSON line,
    and fail if any worker fails."""
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, stderr=None, text=True))
    out0, _ = procs[0].communicate()
    codes = [procs[0].returncode] + [p.wait() for p in procs[1:]]
    if out0:
        sys.stdout.write(out0)
        sys.stdout.flush()
    bad = [(r, c) for r, c in enumerate(codes) if c != 0]
    if bad:
        print(f"bench.py: worker(s) failed (rank, exit code): {bad}", file=sys.stderr)
        return next(c for _, c in bad) or 1
    return 0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--dtype", default="bf16x", choices=["f16", "bf16", "bf16x"],
                    help="MFMA operand mode: bf16x (default) = bf16 operands in the ResBlock pairs (80 %% of the FLOPs) with f16 residual "
                         "streams, f16 elsewhere: BASELINE.json names bf16 and >= 40 dB; all-bf16 measures 34 dB, bf16x 45.6 dB, f16 52 dB")
    ap.add_argument("--in-flight", type=int, default=2, metavar="N",
                    help="batches in flight per GPU: step i runs on lane i %% N, each lane with its own inputs, workspace, output, "
                         "hipGraph and HIP stream, so the next batch fills the launch tails and dependency gaps of the current "
                         "one (results are bit-identical to one lane; 1 = strictly one batch at a time)")
    ap.add_argument("--settle", type=int, default=40, metavar="S",
                    help="untimed steps at the end of the set-up, before the W warm-up steps, so the device is at its steady clock "
                         "whatever W is (0 = none)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying a hipGraph")
    ap.add_argument("--branches", action="store_true", help="run the three ResBlocks of a stage as parallel graph branches (only stages whose pairs do NOT run fused take that path)")
    ap.add_argument("--debug", action="append", default=[], metavar="NAME=VALUE",
                    help="developer switch of the library (qvc_debug_set), e.g. pair_chain3=1, wn_kernel=1: for A/B runs of variants "
                         "that give identical results; recorded in the JSON line")
    ap.add_argument("--rehearsal", action="store_true",
                    help="developer switch for a 1-GPU box: every rank on cuda:0 with gloo, to exercise the multi-rank control flow")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the waveforms of the last timed step (float32, (batch, 1, samples)) "
                         "to DIR/audio.npy (rank r > 0 of a multi-rank run: DIR/audio_rank<r>.npy); the inputs are seeded, "
                         "so two builds can be compared output for output")
    ap.add_argument("--full", action="store_true",
                    help="also run the diagnostic legs: roofline (per-launch events), steady-state and one-lane windows with "
                         "the lane bit-identity check, speaker-encoder timing, CPU baseline and parity (--no-cpu-baseline "
                         "drops the last two)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_workers(args.gpus, sys.argv[1:], args.rehearsal))

    import torch
    import torch.distributed as dist
    import quickvc_official_amd as q
    from quickvc_official_amd import dist as qd
    from quickvc_official_amd.engine import QvcEngine
    from quickvc_official_amd.synth import make_synthetic_state_dict, make_synthetic_inputs

    exit_code = 0
    rank, local_rank, world = qd.env_world()
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs torch.distributed.run with {args.gpus} processes (WORLD_SIZE={world})")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (the hot path has no CPU fallback)")
    rehearsal = args.rehearsal
    dev_index = 0 if rehearsal else local_rank
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)

    cfg = dict(q.DEFAULT_MODEL_CONFIG)
    model = q.SynthesizerTrn(641, 32, **cfg, operand_dtype=args.dtype)
    # rank 0 owns the checkpoint and packs it; everybody else allocates an empty blob and receives it in ONE broadcast
    sd = make_synthetic_state_dict(model, 1234) if rank == 0 else None
    engine = QvcEngine(model.model_config, sd, device, parallel_branches=args.branches, pack=rank == 0)
    from quickvc_official_amd import lib as qlib
    for kv in args.debug:
        name, _, val = kv.partition("=")
        qlib.debug_set(name, int(val))
    if world > 1:
        qd.broadcast_blob(engine.blob, src=0)                 # RCCL over xGMI, once
    B = args.batch
    n_lanes = max(1, args.in_flight)

    # ---- one step = one batch through the hot path, optionally as a hipGraph (the library call is capturable: no
    #      sync/alloc inside).  A lane owns everything a batch touches -- inputs, workspace (the graph bakes its pointer
    #      in), output, graph, stream -- so consecutive steps on different lanes are independent and may overlap.
    def make_lane(k: int) -> dict:
        u_k, g_k, n_k = make_synthetic_inputs(B, FRAMES, 256, cfg["inter_channels"], cfg["gin_channels"], seed0=(rank + world * k) * B)
        lane = {"unit": u_k.to(device), "g": g_k.to(device), "noise": n_k.to(device), "stream": torch.cuda.Stream(device), "graph": None,
                "out": torch.empty(B, 1, FRAMES * engine.samples_per_frame, dtype=torch.float32, device=device),
                "ws": engine.alloc_workspace(B, FRAMES)}
        with torch.cuda.stream(lane["stream"]):
            engine.infer_batch(lane["unit"], lane["g"], lane["noise"], lane["out"], ws=lane["ws"])       # loads code objects
            lane["stream"].synchronize()
            if not args.no_graph:
                lane["graph"] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(lane["graph"], stream=lane["stream"]):
                    engine.infer_batch(lane["unit"], lane["g"], lane["noise"], lane["out"], ws=lane["ws"])
        return lane

    def run_lane(lane: dict) -> None:
        with torch.cuda.stream(lane["stream"]):
            if lane["graph"] is not None:
                lane["graph"].replay()
            else:
                engine.infer_batch(lane["unit"], lane["g"], lane["noise"], lane["out"], ws=lane["ws"])

    lanes = [make_lane(0)]
    unit, g, noise, out, stream, graph = (lanes[0][key] for key in ("unit", "g", "noise", "out", "stream", "graph"))
    agg, reps, total_ms = {}, 5, 0.0
    if args.full and rank == 0:
        # ---- roofline leg, BEFORE a second lane exists: per-launch HIP events on lane 0's stream (qvc_infer_batch_timed),
        #      same workload, chip at its steady clock.  (Taken after the two-lane windows the very same eager launches
        #      measured 10 % longer -- 249 vs 225 us for the dominant kernel, rocprofv3 of the one-lane run: 225 us.)
        for _ in range(25):                                 # the clock ramp (tools/warmup_probe.py)
            run_lane(lanes[0])
        with torch.cuda.stream(stream):
            # 9 repetitions, the 5 with the smallest step total are kept: one disturbed repetition (seen once on a pool
            # box: the stage-1 pairs 37 % slower for a moment) would otherwise name the wrong dominant kernel
            runs = [engine.infer_batch_timed(unit, g, noise, out)[1] for _ in range(reps + 4)]
        runs.sort(key=lambda recs: sum(r["ms"] for r in recs))
        for recs in runs[:reps]:
            for r in recs:
                a = agg.setdefault(r["name"], {"ms": 0.0, "flops": 0.0, "bytes": 0.0, "launches": 0})
                a["ms"] += r["ms"]; a["flops"] += r["flops"]; a["bytes"] += r["bytes"]; a["launches"] += 1
                total_ms += r["ms"]
        torch.cuda.synchronize()
    lanes += [make_lane(k) for k in range(1, n_lanes)]
    step_no = [0]

    def step(in_flight=n_lanes):
        run_lane(lanes[step_no[0] % in_flight])
        step_no[0] += 1

    # Part of the set-up, not of the W warm-up steps: building the lanes (allocation, capture) leaves the device idle long
    # enough for its clock to drop, and it needs ~20 steps (~45 ms) to come back (tools/warmup_probe.py).  Without this the
    # K timed steps after a handful of warm-up steps measure that ramp (1.88 vs 1.82 ms); `steady_state` below stays as
    # the cross-check.
    for _ in range(args.settle):
        step()
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    if args.dump_outputs:
        # what a caller of the timed path receives from its last step: that lane's waveforms (the other lanes hold the
        # same path's output for their own inputs).  10 MB at batch 32; larger batches keep their first utterances.
        import numpy as np
        last = lanes[(step_no[0] - 1) % n_lanes]["out"]
        per_utt = last[0].numel() * 4
        keep = max(1, min(last.shape[0], (64 << 20) // per_utt))
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "audio.npy" if rank == 0 else f"audio_rank{rank}.npy"),
                last[:keep].float().cpu().numpy())
    if args.full:
        # A second window of K steps, 40 steps later, is reported next to `value` as `steady_state`: the two agree when
        # the settle steps above did their job (with --settle 0 `value` contains the clock ramp: 2.24, 2.50, 2.35, 2.25,
        # 2.16 ... -> 1.98 ms per step, tools/warmup_probe.py).
        for _ in range(40):
            step()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        wall_steady = time.perf_counter() - t1
        # strictly one batch at a time, for comparison (and what the per-kernel profile under profiles/ is taken on)
        wall_single = wall_steady
        lanes_identical = True
        if n_lanes > 1:
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            for _ in range(args.steps):
                step(1)
            torch.cuda.synchronize()
            wall_single = time.perf_counter() - t2
            # overlap must not change a single bit: every lane's output against the same graph run alone
            for lane in lanes:
                before = lane["out"].clone()
                run_lane(lane)
                torch.cuda.synchronize()
                lanes_identical = lanes_identical and bool(torch.equal(before, lane["out"]))
    wall = qd.max_over_ranks(wall, device)
    if args.full:
        wall_steady = qd.max_over_ranks(wall_steady, device)
        wall_single = qd.max_over_ranks(wall_single, device)
    samples_per_step = world * B * FRAMES * engine.samples_per_frame
    value = samples_per_step * args.steps / wall
    ms_per_step = wall / args.steps * 1e3

    result = {
        "metric": "audio samples/sec (16 kHz, 5 s utterances, batch 32 per GPU, whole hot path)",
        "value": value, "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": "batch=32 offline VC, 5 s 16 kHz utterances, 1xMI355X per rank (BASELINE.json configs[2])",
                   "batch_per_gpu": B, "frames": FRAMES, "samples_per_utterance": FRAMES * engine.samples_per_frame,
                   "operands": {"f16": "f16 MFMA operands, fp32 accumulate", "bf16": "bf16 MFMA operands, fp32 accumulate",
                                "bf16x": "bf16 MFMA operands in the fused ResBlock pairs (80 % of the FLOPs) with an f16 residual stream, f16 operands elsewhere, fp32 accumulate"}[args.dtype], "hipgraph": graph is not None,
                   "parallel_resblock_branches": False,     # set below from the launch records: only unfused stages fork
                   "parallelism": f"utterance-sharded x{world}, no per-step collective",
                   "batches_in_flight": n_lanes,
                   **({"debug_switches": args.debug} if args.debug else {})},
        "rtf": wall / args.steps / (world * B * FRAMES * engine.samples_per_frame / SAMPLE_RATE),
        "settle_steps": args.settle,
    }
    if args.full:
        result["steady_state"] = {
            "ms_per_step": wall_steady / args.steps * 1e3, "value": samples_per_step * args.steps / wall_steady,
            "note": f"the same {args.steps} steps timed again after 40 more steps (device at its steady clock); "
                    "`value` is the first window, right after the settle + warm-up steps"}
        result["one_batch_at_a_time"] = {
            "ms_per_step": wall_single / args.steps * 1e3, "value": samples_per_step * args.steps / wall_single,
            "note": "the same graphs replayed on one lane only (steady clock); the per-launch durations of the "
                    "roofline leg and of the rocprofv3 summary are taken in this mode",
            "lanes_bit_identical_to_running_alone": lanes_identical}

    if rank == 0:
        # the fork / join path exists only for stages whose ResBlock pairs do not run fused (qvc_plan_info()[7])
        import ctypes
        info = (ctypes.c_int32 * 8)()
        engine.lib.qvc_plan_info(ctypes.byref(engine.cfg), info)
        result["config"]["parallel_resblock_branches"] = bool(args.branches and not info[7])
        if args.branches and info[7]:
            print("bench.py: --branches has no effect on this configuration (every stage runs its three chains fused in one launch)", file=sys.stderr)
    if args.full and rank == 0:
        # ---- roofline leg: measured above, before the second lane was built (per-launch HIP events on the launch stream)
        dom_name, dom = max(agg.items(), key=lambda kv: kv[1]["ms"])
        achieved = dom["flops"] / (dom["ms"] * 1e-3) / 1e12 if dom["ms"] > 0 else 0.0
        # HBM traffic per launch comes from separate rocprofv3 --pmc passes (tools/profile_bench.sh writes
        # profiles/r03_traffic.json with the hash of the kernel sources it was measured on).  It is reported only
        # when that hash matches the sources of THIS run and the file names the dominant kernel; otherwise null.
        traffic, traffic_source = None, "no PMC file for these kernel sources (run tools/profile_bench.sh)"
        tpath = os.path.join(ROOT, "profiles", "r03_traffic.json")
        if args.batch != BATCH:
            traffic_source = f"the PMC file is for batch {BATCH} per GPU (bytes per launch scale with the batch)"
        elif os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
                if tj.get("kernel_source_sha1") != kernel_source_sha1():
                    traffic_source = f"stale: {os.path.basename(tpath)} was measured on other kernel sources"
                elif dom_name in tj.get("kernels", {}):
                    traffic = tj["kernels"][dom_name]["hbm_bytes_per_launch"]
                    traffic_source = (f"profiles/{os.path.basename(tpath)} (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, "
                                      f"separate passes, same kernel sources)")
            except Exception as exc:
                traffic_source = f"unreadable PMC file: {exc}"
        all_flops = sum(a["flops"] for a in agg.values()) / reps
        result["roofline"] = {
            "bound": "mfma", "kernel": dom_name, "achieved": achieved, "peak": PEAK_MFMA_TFLOPS, "unit": "TFLOP/s",
            "frac": achieved / PEAK_MFMA_TFLOPS, "traffic": traffic, "traffic_source": traffic_source,
            "algorithmic_bytes_per_launch": dom["bytes"] / dom["launches"],
            "launches_per_step": dom["launches"] // reps, "avg_launch_ms": dom["ms"] / dom["launches"],
            "kernel_share_of_step": dom["ms"] / total_ms,
            "whole_step": {"flops": all_flops, "tflops": all_flops / (ms_per_step * 1e-3) / 1e12,
                           "frac_mfma": all_flops / (ms_per_step * 1e-3) / 1e12 / PEAK_MFMA_TFLOPS,
                           "event_sum_ms": total_ms / reps},
            "by_kernel": {k: {"ms_per_step": v["ms"] / reps, "tflops": (v["flops"] / (v["ms"] * 1e-3) / 1e12) if v["ms"] > 0 else 0.0,
                              "gbs": (v["bytes"] / (v["ms"] * 1e-3) / 1e9) if v["ms"] > 0 else 0.0,
                              "launches": v["launches"] // reps} for k, v in sorted(agg.items(), key=lambda kv: -kv[1]["ms"])},
        }

        # ---- the step in front of the path: speaker embeddings of the batch's targets in one call.
        #      Reported beside the metric, never part of `value` (the hot path starts after the speaker encoder).
        try:
            from quickvc_official_amd.synth import make_synthetic_mel
            mel = torch.cat([make_synthetic_mel(FRAMES, 80, seed=9000 + i) for i in range(B)], 0).to(device)
            with torch.cuda.stream(stream):
                for _ in range(2):
                    engine.speaker_embed(mel)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(10):
                    engine.speaker_embed(mel)
                e1.record(stream)
            stream.synchronize()
            result["speaker_encoder"] = {"ms_per_call": e0.elapsed_time(e1) / 10, "utterances": B, "mel_frames": FRAMES,
                                         "kernel": "3 x (input-projection conv + persistent LSTM launch) + embed"}
        except Exception as exc:                                  # diagnostics only: never fail the bench line
            result["speaker_encoder"] = {"error": str(exc)[:200]}

        # ---- parity + CPU baseline on a bounded sample of the same workload (oracle = checker / baseline only)
        if world == 1 and not args.no_cpu_baseline:
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
            import qvc_oracle as oracle
            avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
            cores = min(avail, 16)          # the 1-GPU box's CPU share; more threads only oversubscribe
            torch.set_num_threads(cores)
            n_cpu, passes = B, 6          # the whole batch, ~10-20 s of CPU work in total
            u_c, g_c, n_c = unit[:n_cpu].cpu(), g[:n_cpu].cpu(), noise[:n_cpu].cpu()
            oracle.infer_from_g(sd, cfg, u_c[:2], g_c[:2].unsqueeze(-1), n_c[:2])          # warm-up
            walls = []
            for _ in range(passes):
                t0 = time.perf_counter()
                ref = oracle.infer_from_g(sd, cfg, u_c, g_c.unsqueeze(-1), n_c)
                walls.append(time.perf_counter() - t0)
            cpu_wall = sorted(walls)[len(walls) // 2]
            snrs = [oracle.snr_db(ref[i], out[i].cpu()) for i in range(n_cpu)]
            result["cpu_baseline"] = {
                "value": n_cpu * FRAMES * engine.samples_per_frame / cpu_wall, "unit": "samples/s", "cores": cores,
                "kind": "port", "sample": f"the same {n_cpu} x 5 s utterances, fp32 CPU oracle (torch, {cores} threads), "
                                          f"1 warm-up + median of {passes} timed passes",
                "wall_s": cpu_wall}
            result["parity"] = {"snr_db_min": min(snrs), "snr_db_mean": sum(snrs) / len(snrs),
                                "linf": float((ref - out[:n_cpu].cpu()).abs().max()), "tolerance_db": 40.0,
                                "checked_utterances": n_cpu}
    if rank == 0:
        print(json.dumps(result))
        par = result.get("parity")
        if par and not (par["snr_db_min"] >= par["tolerance_db"]):
            print(f"PARITY FAILURE: min SNR {par['snr_db_min']:.2f} dB < {par['tolerance_db']} dB", file=sys.stderr)
            exit_code = 3
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if exit_code:
        sys.exit(exit_code)


if __name__ == "__main__":
    main()
