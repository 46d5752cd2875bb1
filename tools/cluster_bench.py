#!/usr/bin/env python3
"""Cluster statistics of many items through Context.batch_clusters (one
workgroup per item, one launch), through the single-path loop (occupy / label
/ label_numbers per item, the only route before the batch call) and, as a
floor, the same trials through Context.batch_scan, in one process on one GPU.
Each item is its own trial (its own shuffled orders) at a fixed point.  The
orders are drawn before the clock starts; a timed batch call includes the rank
arrays' upload and the read-back of the records and the histogram rows, a
timed loop every host call of its items.  A scan trial runs ceil(log2 N) + 2
labelings and an item here one, so the batch call's items/s must reach the
scan's trials/s (`meets_scan_floor`).  After one warm-up of each the legs are
timed alternately `repeats` times; the record keeps every wall time, the best
of each and the spreads.  The loop leg takes at most --loop-cap items (its
rate is per item).

  python tools/cluster_bench.py [--L 50,128 --items 256,1024 --repeats 5 --out DIR]
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
    ap.add_argument("--L", default="50,128")
    ap.add_argument("--items", default="256,1024")
    ap.add_argument("--kinds", default="bond,site,mixed")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nexact", type=int, default=64)
    ap.add_argument("--loop-cap", type=int, default=128)
    ap.add_argument("--pb", type=float, default=0.5, help="bond case")
    ap.add_argument("--ps", type=float, default=0.6, help="site case")
    ap.add_argument("--mixed", default="0.90,0.65", help="mixed case: ps,pb")
    ap.add_argument("--out", default=None, help="directory for batch_clusters_<kind>_L<L>_n<items>.json")
    args = ap.parse_args()
    from percolation_amd import _lib as L
    from percolation_amd import api
    mps, mpb = (float(x) for x in args.mixed.split(","))
    sizes = [int(x) for x in args.items.split(",")]
    nmax = max(sizes)
    for Ls in (int(x) for x in args.L.split(",")):
        with api.Context(0, Ls, Ls, 0) as ctx:
            t, nb = ctx.t, ctx.nb
            tseed = api.trial_seeds(58302, nmax)
            sseed, bseed = api.paired_seeds(8811064, nmax)
            cases = dict(
                bond=(L.BOND, dict(pb=args.pb), 0, int(args.pb * nb), None,
                      lambda: np.stack([api.shuffled_ids(nb, int(s)) for s in tseed])),
                site=(L.SITE, dict(ps=args.ps), int(args.ps * t), 0,
                      lambda: np.stack([api.shuffled_ids(t, int(s)) for s in tseed]), None),
                mixed=(L.SITEBOND, dict(ps=mps, pb=mpb), int(mps * t), int(mpb * nb),
                       lambda: np.stack([api.shuffled_ids(t, int(s)) for s in sseed]),
                       lambda: np.stack([api.shuffled_ids(nb, int(s)) for s in bseed])))
            for name in args.kinds.split(","):
                kind, point, ns, nbc, mk_s, mk_b = cases[name]
                so = mk_s() if mk_s else None
                bo = mk_b() if mk_b else None

                def batch(n):
                    return ctx.batch_clusters(kind, np.arange(n, dtype=np.int32),
                                              site_orders=None if so is None else so[:n],
                                              bond_orders=None if bo is None else bo[:n],
                                              item_nsites=None if so is None else np.full(n, ns, np.int32),
                                              item_nbonds=None if bo is None else np.full(n, nbc, np.int32),
                                              nexact=args.nexact)

                def loop(n):
                    out = []
                    for i in range(n):
                        ctx.occupy(kind, site_order=None if so is None else so[i], nsites=ns,
                                   bond_order=None if bo is None else bo[i], nbonds_=nbc)
                        li = ctx.label()
                        nums = ctx.label_numbers(kind)
                        out.append((li["nclusters"], li["nspan"], nums["maxcs"]))
                    return out

                def scan(n):
                    if kind == L.SITEBOND:
                        return ctx.batch_scan(kind, site_orders=so[:n], bond_orders=bo[:n], scan=L.BOND, fixed=ns)
                    return ctx.batch_scan(kind, site_orders=None if so is None else so[:n],
                                          bond_orders=None if bo is None else bo[:n])

                for n in sizes:
                    nl = min(n, args.loop_cap)
                    batch(n)  # warm-up of every leg at this size
                    loop(min(nl, 16))
                    scan(n)
                    wb, wl, ws = [], [], []
                    for _ in range(args.repeats):
                        t0 = time.perf_counter()
                        recs, hist = batch(n)
                        wb.append(time.perf_counter() - t0)
                        t0 = time.perf_counter()
                        ol = loop(nl)
                        wl.append(time.perf_counter() - t0)
                        t0 = time.perf_counter()
                        scan(n)
                        ws.append(time.perf_counter() - t0)
                    # the two routes saw the same items (the mixed kind's maxcs is
                    # the replay's running maximum: not compared)
                    bad = sum(not (r["nclusters"] - r["nlone"] == ncl and r["nspan"] == nspan
                                   and (name == "mixed" or r["maxcs"] == maxcs))
                              for r, (ncl, nspan, maxcs) in zip(recs, ol))
                    items_s, scan_s = n / min(wb), n / min(ws)
                    rec = dict(
                        workload="cluster_bench square %dx%d %s" % (Ls, Ls, name), kind=name, point=point,
                        items=n, nexact=args.nexact, repeats=args.repeats, loop_items=nl,
                        batch_wall_ms=[round(w * 1e3, 3) for w in wb],
                        loop_wall_ms=[round(w * 1e3, 3) for w in wl],
                        scan_wall_ms=[round(w * 1e3, 3) for w in ws],
                        batch_items_per_s=round(items_s, 1), loop_items_per_s=round(nl / min(wl), 1),
                        scan_trials_per_s=round(scan_s, 1),
                        ratio_vs_loop=round((min(wl) / nl) / (min(wb) / n), 2),
                        ratio_vs_scan=round(items_s / scan_s, 2), meets_scan_floor=bool(items_s >= scan_s),
                        batch_spread=round((max(wb) - min(wb)) / min(wb), 3),
                        loop_spread=round((max(wl) - min(wl)) / min(wl), 3),
                        scan_spread=round((max(ws) - min(ws)) / min(ws), 3),
                        loop_mismatches=int(bad),
                        spanning_share=round(float((recs["nspan"] > 0).mean()), 4),
                        mean_nclusters=round(float(recs["nclusters"].mean()), 1),
                        mean_S=round(float((recs["s2"] / np.maximum(recs["s1"], 1)).mean()), 2))
                    print(json.dumps(rec), flush=True)
                    if args.out:
                        os.makedirs(args.out, exist_ok=True)
                        fn = "batch_clusters_%s_L%d_n%d.json" % (name, Ls, n)
                        with open(os.path.join(args.out, fn), "w") as f:
                            json.dump(rec, f, indent=1)
                            f.write("\n")


if __name__ == "__main__":
    main()
