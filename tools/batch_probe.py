#!/usr/bin/env python3
"""One perc_batch_bondc call over the bond_cond grid of T trials: wall time
per item, the share of items several clusters span (the host fallback), and
the workgroup geometry in force (PERC_BATCH_THREADS=256|512|1024 overrides
the default where 8 rows per thread still cover the system).

  python tools/batch_probe.py [--L 50 --trials 8 --repeats 3 --literal]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", default="50")
    ap.add_argument("--trials", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--literal", action="store_true")
    args = ap.parse_args()
    from percolation_amd import _lib as L
    from percolation_amd import api
    for L_ in map(int, args.L.split(",")):
        with api.Context(0, L_, L_, 0) as ctx:
            if args.literal:
                ctx.set_dot_order(L.DOT_LITERAL)
            nb = ctx.nb
            seeds = api.trial_seeds(58302, args.trials)
            orders = np.stack([api.shuffled_ids(nb, int(s)) for s in seeds])
            grid = sorted({int(c) for c in api.pb_grid(0, nb) if 0 < c <= nb})
            it = np.repeat(np.arange(args.trials, dtype=np.int32), len(grid))
            ic = np.tile(np.array(grid, np.int32), args.trials)
            ctx.batch_bondc(orders, it[:2], ic[:2])  # warm-up
            walls = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                out = ctx.batch_bondc(orders, it, ic)
                walls.append(time.perf_counter() - t0)
            n = len(out)
            print(json.dumps(dict(
                workload="perc_batch_bondc square L=%d" % L_, items=n, trials=args.trials,
                threads=os.environ.get("PERC_BATCH_THREADS", "default"),
                dot="literal" if args.literal else "fast",
                wall_ms=[round(w * 1e3, 3) for w in walls],
                us_per_item=round(min(walls) * 1e6 / n, 2),
                fallback_share=round(sum(o["fallback"] for o in out) / n, 4),
                spanning_share=round(sum(o["nspan"] > 0 for o in out) / n, 4),
                mean_iter=round(sum(o["iter"] for o in out) / n, 1))), flush=True)


if __name__ == "__main__":
    main()
