#!/bin/bash
# the kernel trace summary of a 2-step bench (K = 1, no in-flight leg)
OUT=${OUT:-bench_out}; export OUT; mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/po_prof -o bench -- python3 -u bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --inflight 0 > $OUT/po_prof.log 2>&1 || { tail -20 $OUT/po_prof.log; exit 1; }
rm -f $OUT/po_prof/bench_kernel_trace.csv
