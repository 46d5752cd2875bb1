#!/bin/bash
# the default bench line and the kernel trace summary of a 2-step bench
OUT=${OUT:-bench_out}; export OUT; mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 400 python -u bench.py --full > $OUT/bp_bench.log 2>&1 || { tail -20 $OUT/bp_bench.log; exit 1; }
grep "^{" $OUT/bp_bench.log | tail -1 | cut -c1-200
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/bp_prof -o bench -- python3 -u bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --inflight 0 > $OUT/bp_prof.log 2>&1 || { tail -20 $OUT/bp_prof.log; exit 1; }
rm -f $OUT/bp_prof/bench_kernel_trace.csv
