#!/usr/bin/env bash
# phase probe of the resident solve (PERC_RES_TRACE): L = 1024 with
# and L = 2048; one realisation each
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}" || exit 2
OUT=${OUT:-bench_out}; export OUT; mkdir -p "$OUT"
rm -f $OUT/res_trace_*.csv
for cfg in "1024 1024" "2048 1024"; do
  set -- $cfg
  PERC_RES_TRACE=$OUT/res_trace_$1_$2.csv timeout -k 10 200 python bench.py --full --L $1 --p 0.6 \
    --steps 1 --warmup 0 --no-cpu-baseline > $OUT/res_trace_$1_$2.log 2>&1 || exit 1
done
