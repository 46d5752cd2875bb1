#!/bin/bash
# config 5 as stated, one and two realisations in flight
OUT=${OUT:-bench_out}; export OUT; mkdir -p "$OUT"
export TMPDIR=/tmp
C5="--L 8192 --kind sitebond --ps 0.593 --p 0.50 --no-cpu-baseline"
timeout -k 10 200 python -u bench.py --full $C5 --steps 32 --warmup 1 > $OUT/c5_k1.log 2>&1 || { tail -5 $OUT/c5_k1.log; exit 1; }
timeout -k 10 200 python -u bench.py --full $C5 --steps 64 --warmup 2 --concurrent 2 > $OUT/c5_k2.log 2>&1 || { tail -5 $OUT/c5_k2.log; exit 1; }
for k in 1 2; do grep "^{" $OUT/c5_k$k.log | tail -1 | python3 -c "import json,sys; j=json.load(sys.stdin); print($k, j['value'], j['labeling']['label'])"; done
