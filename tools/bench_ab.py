#!/usr/bin/env python3
"""Interleaved A/B of the bench itself: a probe build of the parent commit
(percolation_amd/probe/libperc_parent.so, PERC_LIBPERC) against the tree's
library, one `bench.py --gpus 1 --steps S --warmup 1 --no-cpu-baseline
--inflight 0 --dump-outputs DIR` process per library and round, parent first.
Stops at the first failing child.  Writes $OUT/<name> (OUT defaults to
bench_out, name to front_ab_L4096.json): every round's figures, whether the
dumped gtop / gbot / iter / nspan files of each round's pair are identical
byte for byte, whether every round of the result beats every round of the
parent, and whether the result's median is within the parent's own spread of
the parent's median.

  python tools/bench_ab.py [rounds=5] [steps=3] [name=front_ab_L4096.json]
"""
import filecmp
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, os.environ.get("OUT", "bench_out"))
os.makedirs(OUT, exist_ok=True)
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
STEPS = sys.argv[2] if len(sys.argv) > 2 else "3"
NAME = sys.argv[3] if len(sys.argv) > 3 else "front_ab_L4096.json"
PARENT = os.path.join(REPO, "percolation_amd", "probe", "libperc_parent.so")
KEYS = ("value", "cg_solves_per_s", "cg_iterations_mean", "cg_solves")
res = {"parent": [], "result": []}
same = []
for r in range(ROUNDS):
    for name in ("parent", "result"):
        env = dict(os.environ)
        if name == "parent":
            env["PERC_LIBPERC"] = PARENT
        d = os.path.join(OUT, "front_dump_%s_%d" % (name, r))
        cmd = [sys.executable, "-u", "bench.py", "--gpus", "1", "--steps", STEPS, "--warmup", "1",
               "--no-cpu-baseline", "--inflight", "0", "--dump-outputs", d]
        p = subprocess.run(["timeout", "-k", "10", "150"] + cmd, cwd=REPO, env=env, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-3000:])
            sys.exit("bench %s round %d rc=%d" % (name, r, p.returncode))
        o = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        rec = {k: o.get(k) for k in KEYS}
        rec["iteration_ms"] = o["cg_iteration"]["ms"]
        rec["kernels"] = {k: v.get("avg_launch_ms") for k, v in o.get("cg_kernels", {}).items() if isinstance(v, dict)}
        res[name].append(rec)
        print(name, r, json.dumps(rec), flush=True)
    a, b = (os.path.join(OUT, "front_dump_%s_%d" % (n, r)) for n in ("parent", "result"))
    files = sorted(os.listdir(a))
    ok = files == sorted(os.listdir(b)) and all(filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False)
                                                for f in files)
    same.append(dict(round=r, files=files, identical=bool(ok)))
pv, rv = [x["value"] for x in res["parent"]], [x["value"] for x in res["result"]]
med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else sum(sorted(v)[len(v) // 2 - 1:len(v) // 2 + 1]) / 2
out = dict(L=4096, steps=int(STEPS), warmup=1, rounds=res, dumps=same,
           parent_value=[min(pv), max(pv)], result_value=[min(rv), max(rv)],
           every_result_round_beats_every_parent_round=min(rv) > max(pv),
           parent_median=med(pv), result_median=med(rv), parent_spread=max(pv) - min(pv),
           result_median_within_parent_spread=med(rv) >= med(pv) - (max(pv) - min(pv)),
           dumps_identical=all(s["identical"] for s in same))
with open(os.path.join(OUT, NAME), "w") as f:
    json.dump(out, f)
    f.write("\n")
print(json.dumps({k: out[k] for k in ("parent_value", "result_value", "every_result_round_beats_every_parent_round",
                                      "parent_median", "result_median", "result_median_within_parent_spread",
                                      "dumps_identical")}))
