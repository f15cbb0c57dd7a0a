#!/bin/bash
# Socket power, clock and temperature (rocm-smi, every 0.5 s) while (a) the bench runs 4000 steps, (b) tools/conv_bench
# runs only the WaveNet stack launches, (c) only the ResBlock pairs -- each for a few seconds.  Run on the GPU box.
# The bench runs with --full, so its timed, steady-state and one-lane windows keep the device busy through the samples.
#   usage: tools/power_probe.sh [OUTDIR]        (default profile_out, relative to the repository root)
cd "$(dirname "$0")/.."
OUT=${1:-profile_out}
mkdir -p $OUT
sample() {   # $1 = output file, $2 = number of samples
  for i in $(seq 1 $2); do rocm-smi --showpower --showclocks --showtemp --json 2>/dev/null | tr -d '\n'; echo; sleep 0.5; done > $1
}
rocm-smi --showpower --showclocks --showtemp > $OUT/smi_idle.txt 2>&1
sample $OUT/smi_bench.txt 24 & S=$!
timeout -k 10 200 python bench.py --full --steps 4000 --warmup 5 --no-cpu-baseline > $OUT/bench_power.json 2> $OUT/bench_power.err
wait $S
sleep 2
sample $OUT/smi_wn.txt 14 & S=$!
QVC_BENCH_WN=1 timeout -k 10 100 ./tools/conv_bench 32 8000 > $OUT/power_wn.txt 2>&1
wait $S
sleep 2
sample $OUT/smi_pairs.txt 30 & S=$!
QVC_BENCH_PAIRS=1 timeout -k 10 100 ./tools/conv_bench 32 1500 > $OUT/power_pairs.txt 2>&1
wait $S
echo done
