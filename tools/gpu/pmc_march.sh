#!/bin/bash
# SQ counters of the march kernels (k_cg_march P and B at L = 4096, the
# dispatch set of tools/pmc_probe.py), one counter group per pass and no
# tracing alongside.  TAG names the output, PERC_LIBPERC picks a probe build:
#   TAG=parent PERC_LIBPERC=percolation_amd/probe/libperc_parent.so tools/gpu/pmc_march.sh
OUT=${OUT:-bench_out}; TAG=${TAG:-main}; L=${L:-4096}
mkdir -p "$OUT"
export TMPDIR=/tmp
i=0
for ctrs in "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_BUSY_CYCLES SQ_WAVE_CYCLES" \
            "SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_ANY SQ_WAIT_ANY GRBM_GUI_ACTIVE"; do
  i=$((i + 1))
  rm -rf "$OUT/pmc_march_$TAG/p$i"
  timeout -k 10 150 rocprofv3 --pmc $ctrs --kernel-include-regex "k_cg_march" -f csv -d "$OUT/pmc_march_$TAG/p$i" -o run \
    -- python3 tools/pmc_probe.py --L "$L" --copies 1 > "$OUT/pmc_march_${TAG}_p$i.log" 2>&1
  rc=$?
  echo "pass $i rc=$rc"
  if [ $rc -ne 0 ]; then tail -20 "$OUT/pmc_march_${TAG}_p$i.log"; exit $rc; fi
done
python3 tools/pmc_march_summary.py "$OUT/pmc_march_$TAG"/p* | tee "$OUT/pmc_march_${TAG}_L$L.txt"
