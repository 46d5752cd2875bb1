#!/usr/bin/env python3
"""Per-launch durations of the march P and B by CG iteration, from the
per-dispatch csv of `rocprofv3 --kernel-trace --stats --output-format csv --
python3 bench.py ...` (a trace run of its own).  A solve starts at k_cg_init;
its n-th k_cg_march<1, ...> launch is P of iteration n, its n-th
k_cg_march<2, ...> launch B's.  Windows of 10 iterations (mean / min / max over
the trace's solves, us) and every 250th iteration up to 8000.

  python tools/march_front_trace.py <kernel_trace.csv> <out.json>
"""
import csv
import json
import sys

path, outp = sys.argv[1], sys.argv[2]
rows = []
with open(path, newline="") as f:
    rd = csv.DictReader(f)
    for r in rd:
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
WIN = {100: (95, 105), 500: (495, 505), 1000: (995, 1005), 2000: (1995, 2005), 3000: (2995, 3005), 3900: (3895, 3905),
       4200: (4195, 4205), 6000: (5995, 6005), 12000: (11995, 12005), 20000: (19995, 20005)}
acc = {kb: {w: [] for w in WIN} for kb in "PB"}
allk = {kb: {} for kb in "PB"}  # per-iteration sums over solves (coarse profile, every 100th)
k = {"P": 0, "B": 0}
solves = 0
for s, e, name in rows:
    if "k_cg_init" in name:
        k = {"P": 0, "B": 0}
        solves += 1
    elif "k_cg_march" in name:
        kb = "P" if "k_cg_march<1," in name else ("B" if "k_cg_march<2," in name else None)
        if kb is None:
            continue
        k[kb] += 1
        d = (e - s) / 1e3
        for w, (lo, hi) in WIN.items():
            if lo <= k[kb] < hi:
                acc[kb][w].append(d)
        if k[kb] % 250 == 0 and k[kb] <= 8000:
            allk[kb].setdefault(k[kb], []).append(d)
out = dict(solves=solves, unit="us", windows={kb: {str(w): dict(n=len(v), mean=round(sum(v) / len(v), 2), min=round(min(v), 2),
                                                                max=round(max(v), 2)) for w, v in acc[kb].items() if v}
                                              for kb in "PB"},
           every_250th={kb: {str(i): round(sum(v) / len(v), 2) for i, v in sorted(allk[kb].items())} for kb in "PB"})
with open(outp, "w") as f:
    json.dump(out, f)
    f.write("\n")
print(json.dumps(out["windows"]))
