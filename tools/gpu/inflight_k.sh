#!/bin/bash
# the bench's in-flight leg at k = 3 and 4 realisations in flight
OUT=${OUT:-bench_out}; export OUT; mkdir -p "$OUT"
for k in 3 4; do
  timeout -k 10 400 python -u bench.py --full --no-cpu-baseline --inflight $k > $OUT/if_$k.log 2>&1 || exit $?
  tail -1 $OUT/if_$k.log | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print($k, d['value'], d.get('in_flight'))"
done
