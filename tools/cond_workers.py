#!/usr/bin/env python3
"""bond_cond trials per second on one GPU through perc_ensemble_bond_cond
with W workers (contexts, host threads, streams) per device, and with the
batch path (perc_ensemble_set_batch: about B (trial, grid point) items per
launch of k_batch_cond, one workgroup each; one worker).

  python tools/cond_workers.py [--L 64,128 --trials 16 --workers 1,2,4,8,16
                                --batch 0,64,256,1024 --repeats 3]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", default="64,128")
    ap.add_argument("--trials", type=int, default=16)
    ap.add_argument("--workers", default="1,2,4,8,16")
    ap.add_argument("--batch", default="0", help="items per launch; 0 = the per-trial loop")
    ap.add_argument("--repeats", type=int, default=1)
    args = ap.parse_args()
    from percolation_amd import api
    for L_ in map(int, args.L.split(",")):
        for B in map(int, args.batch.split(",")):
            # the batch path runs one host thread per device: workers = 1
            for W in (map(int, args.workers.split(",")) if B == 0 else [1]):
                with api.Ensemble(0, L_, L_, 0, ndev=1, workers=W, batch=B) as e:
                    e.bond_cond(58302, min(max(W, 2), args.trials))  # warm-up: every context once
                    for rep in range(args.repeats):
                        t0 = time.perf_counter()
                        res, stats = e.bond_cond(58302, args.trials)
                        wall = time.perf_counter() - t0
                        npts = sum(len(t["rows"]) for t in res)
                        print(json.dumps(dict(
                            workload="bond_cond square L=%d (perc_ensemble, 1 GPU)" % L_, workers=W,
                            batch=e.batch, repeat=rep, trials=args.trials,
                            trials_per_s=round(args.trials / wall, 3), points=npts,
                            ms_per_point=round(wall * 1e3 / npts, 3))), flush=True)


if __name__ == "__main__":
    main()
