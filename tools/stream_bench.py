"""BASELINE.json configs[4]: streaming conversion, 64 concurrent streams, hipGraph replay per step.
Times one step of (a) StreamConverter -- incremental, segment rings (qvc_stream_step) -- and (b) ChunkedConverter --
exact windows over the whole path -- against (c) the offline whole-batch conversion of the same number of frames.
With --live, also (d) LiveConverter -- the windowed step with a bounded look-ahead (qvc_live_step) -- at each of the given
look-aheads ("C" = the whole context): StreamConverter and the LiveConverters of a hop are timed in alternating rounds
of one process and the median round is reported; every look-ahead runs in the trimmed form (the default) and in the
plain form (every stage over the whole window).
With --ticks (and --live L[,L...] for the look-aheads), ONLY (e): per (hop, L) the lockstep LiveConverter.step against
TickConverter -- the tick form, qvc_live_tick -- with every slot bringing hop frames, with a seeded half of the slots idle
per tick, and with uniform random counts in [0, hop]; alternating rounds of one process, medians.  The counts of a tick are
copied into the converter's count tensor on the device in front of every replay (inside the timed region, for all three
tick rows).
With --ring-ticks, ONLY (f): per hop the lockstep StreamConverter.step -- the yardstick -- against StreamTickConverter --
the tick form of the segment rings, qvc_stream_tick -- under the same three patterns, timed the same way.
With --migrate, ONLY (g): slot snapshots (qvc_stream_export_slots / _import_slots) between two StreamConverters of
`streams` slots, hop 16 -> 16 and hop 16 -> 320: the device time of one export call plus one import call for 1 slot and for
all slots (events on one stream, median of rounds), the wall time of StreamConverter.move_slot slot by slot and of
move_slots in one call (synchronised at both ends; the freeing of the source slots included), and the step times beside them.
usage: python tools/stream_bench.py [--live L[,L...]] [--ticks | --ring-ticks | --migrate] [streams] [hop_frames ...]"""
import json
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quickvc_official_amd as q  # noqa: E402
from quickvc_official_amd.lib import debug_set  # noqa: E402
from quickvc_official_amd.streaming import ChunkedConverter, LiveConverter, StreamConverter, StreamTickConverter, TickConverter  # noqa: E402
from quickvc_official_amd.synth import make_synthetic_inputs, make_synthetic_state_dict  # noqa: E402


def timed_replays(conv, n=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(conv._stream):
        # random inputs (zero operands let the chip clock ~20 % higher: DESIGN.md), and enough warm-up steps for the
        # rings of an incremental converter to fill with real data
        conv._unit.normal_()
        conv._noise.normal_()
        conv._g.copy_(torch.nn.functional.normalize(torch.rand_like(conv._g), dim=1))
        for _ in range(12):
            conv._graph.replay()
        e0.record(conv._stream)
        for _ in range(n):
            conv._graph.replay()
        e1.record(conv._stream)
    conv._stream.synchronize()
    return e0.elapsed_time(e1) / n


def live_rows(model, streams, hop, looks, rounds=5):
    """ms per step of StreamConverter and of LiveConverter at every look-ahead of `looks`, alternating, median of `rounds`."""
    convs = {"stream": StreamConverter(model, streams, hop_frames=hop)}
    context = model.engine().live_sizes(streams, hop, 0)[2]
    for look in looks:
        L = context if look == "C" else int(look)
        convs[f"live_L{L}"] = LiveConverter(model, streams, hop, L)
        debug_set("live_trim", 0)            # read when the step is issued, i.e. at capture: the plain form of the same step
        convs[f"live_L{L}_plain"] = LiveConverter(model, streams, hop, L)
        debug_set("live_trim", 1)
    ms = {k: [] for k in convs}
    for _ in range(rounds):
        for k, conv in convs.items():
            ms[k].append(timed_replays(conv))
    out = {"context_frames": context}
    for k, conv in convs.items():
        mid = sorted(ms[k])[len(ms[k]) // 2]
        out[k] = {"ms_per_step": mid, "ms_rounds": [round(v, 4) for v in ms[k]], "lag_frames": conv.lag,
                  "window_frames": getattr(conv, "window", None), "us_per_frame": mid * 1e3 / (streams * hop)}
    return out


def timed_ticks(conv, counts, n=20, copy=True):
    """ms per tick of a TickConverter: `counts` (12 + n, streams) int32 on the device, row i = n_new of replay i.
    copy=False: the counts are written once, in front of the warm-up (a pattern that is the same at every tick)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(conv._stream):
        conv._unit.normal_()
        conv._noise.normal_()
        conv._g.copy_(torch.nn.functional.normalize(torch.rand_like(conv._g), dim=1))
        conv._n.copy_(counts[0])
        for i in range(12):
            if copy:
                conv._n.copy_(counts[i])
            conv._graph.replay()
        e0.record(conv._stream)
        for i in range(12, 12 + n):
            if copy:
                conv._n.copy_(counts[i])
            conv._graph.replay()
        e1.record(conv._stream)
    conv._stream.synchronize()
    return e0.elapsed_time(e1) / n


def tick_patterns(streams, hop, n):
    """The three tick patterns of 12 + n replays (seeded per hop): every slot hop frames, a half of the slots idle per tick,
    uniform counts in [0, hop] -> (the lists, the same as int32 device tensors)."""
    rnd = random.Random(1300 + hop)
    pats = {"full": [[hop] * streams for _ in range(12 + n)], "half_idle": [], "uniform": []}
    for _ in range(12 + n):
        idle = set(rnd.sample(range(streams), streams // 2))
        pats["half_idle"].append([0 if s in idle else hop for s in range(streams)])
        pats["uniform"].append([rnd.randint(0, hop) for _s in range(streams)])
    return pats, {k: torch.tensor(v, dtype=torch.int32, device="cuda") for k, v in pats.items()}


def ring_tick_rows(model, streams, hop, rounds=7, n=20):
    """ms per step of StreamConverter (lockstep: the yardstick, its spread over the rounds the margin) and of
    StreamTickConverter under the three tick patterns, alternating, median of `rounds`."""
    pats, dev_pats = tick_patterns(streams, hop, n)
    convs = {"lockstep": StreamConverter(model, streams, hop_frames=hop)}
    for k in pats:
        convs["tick_" + k] = StreamTickConverter(model, streams, hop_frames=hop)
    convs["tick_full_counts_written_once"] = convs["tick_full"]       # the same converter without the copy of the counts per tick
    ms = {k: [] for k in convs}
    for _ in range(rounds):
        for k, conv in convs.items():
            if k == "lockstep":
                ms[k].append(timed_replays(conv, n))
            else:
                once = k.endswith("_written_once")
                ms[k].append(timed_ticks(conv, dev_pats["full" if once else k[5:]], n, copy=not once))
    n_flows = int(model.model_config.get("n_flows", 4))
    row = {"lag_frames": convs["lockstep"].lag,
           "data_movement_launches": {"lockstep_step": f"{5 + n_flows} copy_batch", "tick": f"{5 + n_flows} copy_counted"},
           "mean_frames_per_slot_and_tick": {k: sum(map(sum, v[12:])) / (n * streams) for k, v in pats.items()}}
    for k in convs:
        mid = sorted(ms[k])[len(ms[k]) // 2]
        row[k] = {"ms_per_step": mid, "ms_rounds": [round(v, 4) for v in ms[k]]}
    row["lockstep_spread_ms"] = round(max(ms["lockstep"]) - min(ms["lockstep"]), 4)
    return row


def tick_rows(model, streams, hop, looks, rounds=5, n=20):
    """ms per step of LiveConverter (lockstep) and of TickConverter under three tick patterns, per look-ahead of `looks`,
    alternating, median of `rounds`."""
    context = model.engine().live_sizes(streams, hop, 0)[2]
    pats, dev_pats = tick_patterns(streams, hop, n)
    out = {"context_frames": context,
           "launches_beside_the_path": {"lockstep_step": "3 copy_batch (append; deliver + rings out; rings back)",
                                        "tick": "3 copy_counted (the same three, per-slot counts)"},
           "mean_frames_per_slot_and_tick": {k: sum(map(sum, v[12:])) / (n * streams) for k, v in pats.items()}}
    for look in looks:
        L = context if look == "C" else int(look)
        convs = {"lockstep": LiveConverter(model, streams, hop, L)}
        for k in pats:
            convs["tick_" + k] = TickConverter(model, streams, hop, L)
        ms = {k: [] for k in convs}
        for _ in range(rounds):
            for k, conv in convs.items():
                ms[k].append(timed_replays(conv, n) if k == "lockstep" else timed_ticks(conv, dev_pats[k[5:]], n))
        row = {"window_frames": convs["lockstep"].window}
        for k in convs:
            mid = sorted(ms[k])[len(ms[k]) // 2]
            row[k] = {"ms_per_step": mid, "ms_rounds": [round(v, 4) for v in ms[k]]}
        out[f"L{L}"] = row
        del convs
        torch.cuda.empty_cache()
    return out


def migrate_rows(model, streams, src_hop=16, dst_hops=(16, 320), rounds=7, n=10):
    """ms to move 1 slot and all `streams` slots from a hop-`src_hop` converter into converters of `dst_hops`."""
    import time
    from quickvc_official_amd.engine import aligned_empty
    eng = model.engine()
    src = StreamConverter(model, streams, hop_frames=src_hop)
    n_snap = eng.stream_snapshot_bytes()
    res = {"snapshot_bytes_per_slot": n_snap, "snapshot_tag": f"{eng.stream_snapshot_tag():#018x}", "source_hop": src_hop,
           "source_ms_per_step": timed_replays(src)}
    snap = aligned_empty(streams * n_snap, eng.device)
    mid = lambda v: sorted(v)[len(v) // 2]
    for hop in dst_hops:
        dst = StreamConverter(model, streams, hop_frames=hop)
        row = {"dest_ms_per_step": timed_replays(dst)}
        for label, slots in (("1_slot", [streams // 2]), ("all_slots", list(range(streams)))):
            dev_ms, wall_ms, call_ms = [], [], []
            for _ in range(rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(src._stream):
                    e0.record(src._stream)
                    for _i in range(n):
                        eng.stream_export_slots(src._state, streams, src_hop, slots, src._pos, src._len, snap)
                        eng.stream_import_slots(dst._state, streams, hop, slots, dst._pos, dst._len, snap)
                    e1.record(src._stream)
                src._stream.synchronize()
                dev_ms.append(e0.elapsed_time(e1) / n)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for b in slots:
                    src.move_slot(b, dst, b)
                torch.cuda.synchronize()
                wall_ms.append((time.perf_counter() - t0) * 1e3)
                src.reset()                      # the moved slots were freed: all slots live again for the next round
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                src.move_slots(slots, dst, slots)
                torch.cuda.synchronize()
                call_ms.append((time.perf_counter() - t0) * 1e3)
                src.reset()
            row[label] = {"export_plus_import_device_ms": mid(dev_ms), "device_ms_rounds": [round(v, 4) for v in dev_ms],
                          "move_slot_one_by_one_wall_ms": mid(wall_ms), "one_by_one_wall_ms_rounds": [round(v, 4) for v in wall_ms],
                          "move_slots_one_call_wall_ms": mid(call_ms), "one_call_wall_ms_rounds": [round(v, 4) for v in call_ms],
                          "bytes_moved": len(slots) * n_snap}
        res[f"hop_{src_hop}_to_{hop}"] = row
        del dst
        torch.cuda.empty_cache()
    return res


def main():
    argv = sys.argv[1:]
    migrate = "--migrate" in argv
    if migrate:
        argv.remove("--migrate")
    looks = None
    ticks = "--ticks" in argv
    if ticks:
        argv.remove("--ticks")
    ring_ticks = "--ring-ticks" in argv
    if ring_ticks:
        argv.remove("--ring-ticks")
    if "--live" in argv:
        i = argv.index("--live")
        looks = argv[i + 1].split(",")
        del argv[i:i + 2]
    streams = int(argv[0]) if argv else 64
    hops = [int(x) for x in argv[1:]] or [320, 16]
    model = q.SynthesizerTrn(641, 32, **q.DEFAULT_MODEL_CONFIG)
    model.load_state_dict(make_synthetic_state_dict(model, 1234))
    model = model.cuda().eval()
    spf = model.samples_per_frame
    if migrate:
        print(json.dumps({"streams": streams, "migrate": migrate_rows(model, streams)}))
        return
    if ring_ticks:
        res = {"streams": streams, "ring_ticks": {}}
        for hop in hops:
            res["ring_ticks"][str(hop)] = ring_tick_rows(model, streams, hop)
            torch.cuda.empty_cache()
        print(json.dumps(res))
        return
    if ticks:
        res = {"streams": streams, "ticks": {str(hop): tick_rows(model, streams, hop, looks or ["0", "8", "C"]) for hop in hops}}
        print(json.dumps(res))
        return
    # offline cost per frame: the whole batch of `streams` x 320 frames in one call (graph replay)
    eng = model.engine()
    unit, g, noise = make_synthetic_inputs(streams, 320, 256, 192, 256, seed0=500)
    unit, g, noise = unit.cuda(), g.cuda(), noise.cuda()
    out = torch.empty(streams, 1, 320 * spf, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ws = eng.alloc_workspace(streams, 320)
        eng.infer_batch(unit, g, noise, out, ws=ws)
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            eng.infer_batch(unit, g, noise, out, ws=ws)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(10):
            graph.replay()
        e1.record(s)
    s.synchronize()
    offline_us_per_frame = e0.elapsed_time(e1) / 10 * 1e3 / (streams * 320)
    res = {"streams": streams, "offline_us_per_frame": offline_us_per_frame, "offline_ms_per_320_frames": e0.elapsed_time(e1) / 10, "hops": {}}
    for hop in hops:
        inc = StreamConverter(model, streams, hop_frames=hop)
        ms_inc = timed_replays(inc)
        row = {"incremental_ms_per_step": ms_inc, "incremental_us_per_frame": ms_inc * 1e3 / (streams * hop),
               "incremental_vs_offline": ms_inc * 1e3 / (streams * hop) / offline_us_per_frame, "lag_frames": inc.lag,
               "incremental_useful_samples_per_s": streams * hop * spf / (ms_inc * 1e-3),
               "audio_seconds_per_step_per_stream": hop * spf / 16000.0}
        del inc
        try:
            ch = ChunkedConverter(model, streams, hop_frames=hop)
            ms_ch = timed_replays(ch)
            row.update({"windowed_ms_per_step": ms_ch, "windowed_vs_offline": ms_ch * 1e3 / (streams * hop) / offline_us_per_frame,
                        "windowed_window_frames": ch.window})
            del ch
        except Exception as exc:                      # e.g. out of memory at a tiny hop x many streams
            row["windowed_error"] = str(exc)[:120]
        if looks is not None:
            torch.cuda.empty_cache()
            row["live"] = live_rows(model, streams, hop, looks)
        res["hops"][str(hop)] = row
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
