#!/usr/bin/env python3
"""Throughput of the §8(f) callers around the hot path on one GPU:

  bond_perc / site_perc (threshold scans, Square/bond_perc.f:86-369,
    site_perc.f:69-260): per trial the reference shuffle (host), the first
    spanning occupation count by GPU bisection (perc_first_spanning, ~log2 N
    labelings), the largest and spanning cluster sizes at that count
    (perc_cluster_sizes, GPU);
  bond_cond (Square/bond_cond.f:123-498): per trial one labeling +
    conductance solve at each of the ~100 grid points, then the pc scan.

Prints one JSON line per workload: trials/s and the per-trial split.

  python tools/scan_bench.py [--L 256,1024 --trials 8 --cond-L 64,256 --cond-trials 2]

With --batch N (lattices perc_scan_supported accepts) each bond_perc /
site_perc workload is timed three times in the same process, the shuffles
included, --reps times in alternation: the per-trial path above, the batch
path (the orders of N trials at a time shuffled on the host, one
perc_batch_scan call per group: one workgroup bisects each trial) and the
seeded batch path (the same groups through perc_batch_scan_seeded: the orders
shuffled on the device, one wave per trial, no host shuffle and no upload).
Prints the three trials/s (medians), the ratios, every repetition's seconds
and whether the three paths' records agree; bond_cond is not run.
--no-per-trial leaves the per-trial leg out (sweeps of --batch for the
crossover of the two batch legs).

  python tools/scan_bench.py --L 50 --trials 1000 --batch 256
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def scan(api, L_mod, lat, L_, kind, trials):
    N = api.nbonds(lat, L_, L_, 0) if kind == L_mod.BOND else L_ * L_
    seeds = api.trial_seeds(58302, trials, scale=1000000)
    t_shuf = t_gpu = t_rep = 0.0
    firsts = []
    with api.Context(lat, L_, L_, 0) as ctx:
        api.first_spanning(ctx, api.shuffled_ids(N, 12345), kind, N)  # warm-up
        t0 = time.perf_counter()
        for ii in range(trials):
            a = time.perf_counter()
            order = api.shuffled_ids(N, int(seeds[ii]))
            b = time.perf_counter()
            first = api.first_spanning(ctx, order, kind, N)
            c = time.perf_counter()
            ctx.cluster_sizes()  # maxcs, spanning size on the GPU (perc_cluster_sizes)
            d = time.perf_counter()
            t_shuf += b - a
            t_gpu += c - b
            t_rep += d - c
            firsts.append(first)
        wall = time.perf_counter() - t0
    return dict(workload="%s_perc %s L=%d" % ("bond" if kind == L_mod.BOND else "site",
                                               "square" if lat == 0 else "triangular", L_),
                trials=trials, trials_per_s=round(trials / wall, 3),
                ms_per_trial=round(wall * 1e3 / trials, 2),
                host_shuffle_ms=round(t_shuf * 1e3 / trials, 2),
                gpu_first_spanning_ms=round(t_gpu * 1e3 / trials, 2),
                gpu_cluster_sizes_ms=round(t_rep * 1e3 / trials, 2),
                mean_first_fraction=round(float(np.mean(firsts)) / N, 5))


def scan_ab(api, L_mod, lat, L_, kind, trials, batch, reps, per_trial_leg=True):
    """the per-trial path, the batch path and the seeded batch path on the
    same trials, alternating"""
    N = api.nbonds(lat, L_, L_, 0) if kind == L_mod.BOND else L_ * L_
    seeds = api.trial_seeds(58302, trials, scale=1000000)
    key = "bond_orders" if kind == L_mod.BOND else "site_orders"
    skey = "bond_seeds" if kind == L_mod.BOND else "site_seeds"

    def per_trial(ctx):
        out = []
        for ii in range(trials):
            order = api.shuffled_ids(N, int(seeds[ii]))
            first = api.first_spanning(ctx, order, kind, N)
            out.append((first,) + ctx.cluster_sizes())
        return out

    def batched(ctx):
        out, t_shuf = [], 0.0
        for i0 in range(0, trials, batch):
            a = time.perf_counter()
            orders = np.stack([api.shuffled_ids(N, int(s)) for s in seeds[i0:i0 + batch]])
            t_shuf += time.perf_counter() - a
            out += [(r["first"], r["maxcs"], r["span_size"]) for r in ctx.batch_scan(kind, **{key: orders})]
        return out, t_shuf

    def seeded(ctx):
        out = []
        for i0 in range(0, trials, batch):
            res = ctx.batch_scan_seeded(kind, **{skey: seeds[i0:i0 + batch]})
            out += [(r["first"], r["maxcs"], r["span_size"]) for r in res]
        return out

    with api.Context(lat, L_, L_, 0) as ctx:
        warm = api.shuffled_ids(N, 12345)
        api.first_spanning(ctx, warm, kind, N)  # warm-up of both paths
        ctx.cluster_sizes()
        ctx.batch_scan(kind, **{key: np.stack([warm] * min(batch, trials))})
        ctx.batch_scan_seeded(kind, **{skey: seeds[:min(batch, trials)]})
        ta, tb, tc, ts = [], [], [], []
        ra = None
        for _ in range(reps):
            t0 = time.perf_counter()
            if per_trial_leg:
                ra = per_trial(ctx)
            t1 = time.perf_counter()
            rb, shuf = batched(ctx)
            t2 = time.perf_counter()
            rc = seeded(ctx)
            t3 = time.perf_counter()
            ta.append(t1 - t0)
            tb.append(t2 - t1)
            tc.append(t3 - t2)
            ts.append(shuf)
    wa, wb, wc = float(np.median(ta)), float(np.median(tb)), float(np.median(tc))
    return dict(workload="%s_perc %s L=%d" % ("bond" if kind == L_mod.BOND else "site",
                                               "square" if lat == 0 else "triangular", L_),
                trials=trials, batch=batch, reps=reps,
                per_trial_trials_per_s=round(trials / wa, 2) if per_trial_leg else None,
                batch_trials_per_s=round(trials / wb, 2),
                seeded_trials_per_s=round(trials / wc, 2),
                ratio=round(wa / wb, 2) if per_trial_leg else None,
                seeded_ratio=round(wb / wc, 2),
                per_trial_s=[round(x, 4) for x in ta] if per_trial_leg else None,
                batch_s=[round(x, 4) for x in tb], seeded_s=[round(x, 4) for x in tc],
                seeded_beats_batch=max(tc) < min(tb),
                batch_host_shuffle_s=round(float(np.median(ts)), 4),
                records_equal=(ra is None or ra == rb) and rb == rc,
                mean_first_fraction=round(float(np.mean([r[0] for r in rb])) / N, 5))


def cond(api, lat, L_, trials):
    with api.Context(lat, L_, L_, 0) as ctx:
        api.bond_cond_grid(lat, L_, L_, 0, numtrials=1, itmax=10 ** 6, ctx=ctx)  # warm-up
        t0 = time.perf_counter()
        out = api.bond_cond_grid(lat, L_, L_, 0, numtrials=trials, itmax=10 ** 6, ctx=ctx)
        wall = time.perf_counter() - t0
    npts = sum(len(t["rows"]) for t in out)
    iters = sum(r["iter"] for t in out for r in t["rows"])
    return dict(workload="bond_cond %s L=%d" % ("square" if lat == 0 else "triangular", L_),
                trials=trials, trials_per_s=round(trials / wall, 4),
                ms_per_trial=round(wall * 1e3 / trials, 1), grid_points=npts,
                points_per_s=round(npts / wall, 2), cg_iterations=iters,
                ms_per_point=round(wall * 1e3 / max(npts, 1), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", default="256,1024")
    ap.add_argument("--trials", type=int, default=8)
    ap.add_argument("--cond-L", default="64,256")
    ap.add_argument("--cond-trials", type=int, default=2)
    ap.add_argument("--batch", type=int, default=0,
                    help="A/B of the per-trial path and perc_batch_scan with this many trials per call")
    ap.add_argument("--reps", type=int, default=3, help="alternating repetitions of the A/B")
    ap.add_argument("--no-per-trial", action="store_true", help="with --batch: the two batch legs only")
    args = ap.parse_args()
    from percolation_amd import _lib as L_mod
    from percolation_amd import api
    if args.batch > 0:
        for L_ in map(int, args.L.split(",")):
            if not api.scan_supported(0, L_, L_, 0):
                raise SystemExit("L=%d: not a lattice perc_scan_supported accepts" % L_)
            for kind in (L_mod.BOND, L_mod.SITE):
                print(json.dumps(scan_ab(api, L_mod, 0, L_, kind, args.trials, args.batch,
                                         args.reps, not args.no_per_trial)), flush=True)
        return
    for L_ in map(int, args.L.split(",")):
        for kind in (L_mod.BOND, L_mod.SITE):
            print(json.dumps(scan(api, L_mod, 0, L_, kind, args.trials)), flush=True)
    for L_ in map(int, args.cond_L.split(",")):
        print(json.dumps(cond(api, 0, L_, args.cond_trials)), flush=True)


if __name__ == "__main__":
    main()
