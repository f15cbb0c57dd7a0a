"""Per-kernel stats and cross-stream overlap of the WaveNet stack launches, from one rocprofv3 --kernel-trace database.

    rocprofv3 --kernel-trace --stats -d DIR -o run -- python3 bench.py --gpus 1 --steps 20 --warmup 5
    python3 tools/kernel_overlap.py DIR/run_results.db [--csv OUT.csv]

Prints, for the wn_stack2 launches, what share of their time some launch of another kernel family runs at the same
moment (two batches in flight: the other lane's decoder), and which families those are.  --csv writes the
kernel-stats summary (name, calls, total / mean / min / max ns, share of the summed kernel time)."""
import argparse
import collections
import csv
import re
import sqlite3


def family(name):
    m = re.match(r"_ZN\d*qvc(\d+)", name)          # mangled: _ZN3qvc16wn_stack2_kernelI...
    if m:
        n = int(m.group(1))
        return name[m.end():m.end() + n]
    m = re.match(r"(?:void )?(?:qvc::)?([a-z0-9_]+)", name)
    return m.group(1) if m else name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("db")
    ap.add_argument("--csv")
    args = ap.parse_args()
    rows = sqlite3.connect(args.db).execute("select name, start, end, queue_id, grid_x, grid_y, grid_z, workgroup_x from kernels").fetchall()
    stats = collections.defaultdict(list)
    for name, s, e, *_ in rows:
        stats[name].append(e - s)
    tot = sum(sum(v) for v in stats.values())
    if args.csv:
        with open(args.csv, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs", "Percentage"])
            for name, v in sorted(stats.items(), key=lambda kv: -sum(kv[1])):
                w.writerow([name, len(v), sum(v), sum(v) / len(v), min(v), max(v), 100.0 * sum(v) / tot])
    wn = [(s, e, q, gx * gy * gz // wx) for n, s, e, q, gx, gy, gz, wx in rows if family(n) == "wn_stack2_kernel"]
    other = sorted((s, e, family(n)) for n, s, e, *_ in rows if family(n) != "wn_stack2_kernel")
    wn_ns, ov_ns, by = 0, 0, collections.Counter()
    for s, e, _q, _wg in wn:
        wn_ns += e - s
        ivs = [(max(s, os_), min(e, oe), f) for os_, oe, f in other if os_ < e and oe > s]
        for a, b, f in ivs:
            by[f] += b - a
        ivs.sort()
        cur_a = cur_b = None
        for a, b, _f in ivs:                      # union of the overlapping intervals
            if cur_b is None or a > cur_b:
                if cur_b is not None:
                    ov_ns += cur_b - cur_a
                cur_a, cur_b = a, b
            else:
                cur_b = max(cur_b, b)
        if cur_b is not None:
            ov_ns += cur_b - cur_a
    print(f"wn_stack2 launches: {len(wn)}, workgroups per launch: {sorted(set(w for *_, w in wn))}, "
          f"mean {wn_ns / max(len(wn), 1) / 1e3:.1f} us")
    print(f"share of wn_stack2 time with another kernel running at the same moment: {ov_ns / max(wn_ns, 1):.3f}")
    for f, ns in by.most_common(6):
        print(f"  {f}: {ns / max(wn_ns, 1):.3f} of wn_stack2 time (summed over launches)")


if __name__ == "__main__":
    main()
