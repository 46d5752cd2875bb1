#!/usr/bin/env python3
"""Conductance items through the large batch kernel (Context.set_batch_large:
one workgroup of 1024 threads per item, p alone in LDS) against another path
on the same occupancies, in one process on one GPU: items/s of both and their
ratio.  --against loop: the single-path loop (occupy / label / conductance
per item), the only other path past 8192 interior rows; --against batch: the
default batch kernel, on a lattice both kernels take.  Each item is its own
trial at a fixed point: bond at pb, site at ps, mixed at (ps, pb).  The
protocol is tools/cond_batch_bench.py's: the orders are drawn before the clock
starts, a timed batch call includes the rank arrays' upload and the read-back,
a timed loop every host call of its items; one warm-up of each, then the two
timed alternately `repeats` times; the record keeps every wall time, the best
of each and the spread.

  python tools/batch_large_bench.py [--m 128 --n 128 --items 256 --against loop --out DIR]
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
    ap.add_argument("--m", type=int, default=128)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--items", default="256")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kinds", default="bond,site,mixed")
    ap.add_argument("--pb", type=float, default=0.60, help="bond case")
    ap.add_argument("--ps", type=float, default=0.66, help="site case")
    ap.add_argument("--mixed", default="0.90,0.80", help="mixed case: ps,pb")
    ap.add_argument("--against", choices=("loop", "batch"), default="loop")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--itmax", type=int, default=20000)
    ap.add_argument("--out", default=None, help="directory for batch_large_<kind>_<m>x<n>_n<items>_vs_<against>.json")
    args = ap.parse_args()
    from percolation_amd import _lib as L
    from percolation_amd import api
    mps, mpb = (float(x) for x in args.mixed.split(","))
    sizes = [int(x) for x in args.items.split(",")]
    nmax = max(sizes)
    with api.Context(0, args.m, args.n, 0) as ctx:
        t, nb = ctx.t, ctx.nb
        tseed = api.trial_seeds(58302, nmax)
        sseed, bseed = api.paired_seeds(8811064, nmax)
        cases = dict(
            bond=(L.BOND, dict(pb=args.pb), 0, int(args.pb * nb), None, tseed),
            site=(L.SITE, dict(ps=args.ps), int(args.ps * t), 0, tseed, None),
            mixed=(L.SITEBOND, dict(ps=mps, pb=mpb), int(mps * t), int(mpb * nb), sseed, bseed))
        for name in args.kinds.split(","):
            kind, point, ns, nbc, ss, bs = cases[name]
            so = None if ss is None else np.stack([api.shuffled_ids(t, int(s)) for s in ss])
            bo = None if bs is None else np.stack([api.shuffled_ids(nb, int(s)) for s in bs])
            rule, cur = api.KIND_RULE[kind], api.natural_cur_rule(kind)

            def batch(n, large):
                ctx.set_batch_large(large)
                try:
                    return ctx.batch_cond(kind, np.arange(n, dtype=np.int32),
                                          site_orders=None if so is None else so[:n],
                                          bond_orders=None if bo is None else bo[:n],
                                          item_nsites=None if so is None else np.full(n, ns, np.int32),
                                          item_nbonds=None if bo is None else np.full(n, nbc, np.int32),
                                          tol=args.tol, itmax=args.itmax)
                finally:
                    ctx.set_batch_large(False)

            def loop(n):
                out = []
                for i in range(n):
                    if kind == L.BOND:
                        ctx.occupy(kind, bond_order=bo[i], nbonds_=nbc)
                    elif kind == L.SITE:
                        ctx.occupy(kind, site_order=so[i], nsites=ns)
                    else:
                        ctx.occupy(kind, site_order=so[i], nsites=ns, bond_order=bo[i], nbonds_=nbc)
                    li = ctx.label()
                    c = ctx.conductance(rule, cur, 1.0, 1.0, api.LEAK, 2, args.tol, args.itmax)
                    out.append(dict(nspan=li["nspan"], gtop=c["gtop"], iter=c["iter"]))
                return out

            other = loop if args.against == "loop" else (lambda n: batch(n, False))
            for n in sizes:
                batch(n, True)  # warm-up of both paths at this size
                other(min(n, 64))
                wb, wo = [], []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    ob = batch(n, True)
                    wb.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    oo = other(n)
                    wo.append(time.perf_counter() - t0)
                # the two paths solved the same items (each in its own fast
                # association: the distance of the two Gtop is recorded)
                worst = 0.0
                for b, o in zip(ob, oo):
                    assert b["nspan"] == o["nspan"], (b, o)
                    if o["gtop"]:
                        worst = max(worst, abs(b["gtop"] - o["gtop"]) / abs(o["gtop"]))
                rec = dict(
                    workload="batch_large_bench square %dx%d %s" % (args.m, args.n, name), kind=name,
                    point=point, items=n, dot="fast", tol=args.tol, itmax=args.itmax, repeats=args.repeats,
                    against=args.against,
                    large_wall_ms=[round(w * 1e3, 3) for w in wb],
                    other_wall_ms=[round(w * 1e3, 3) for w in wo],
                    large_items_per_s=round(n / min(wb), 1), other_items_per_s=round(n / min(wo), 1),
                    ratio=round(min(wo) / min(wb), 3),
                    ratio_median=round(float(np.median(wo) / np.median(wb)), 3),
                    large_spread=round((max(wb) - min(wb)) / min(wb), 3),
                    other_spread=round((max(wo) - min(wo)) / min(wo), 3),
                    spanning_share=round(sum(b["nspan"] > 0 for b in ob) / n, 4),
                    fallback_share=round(sum(b["fallback"] for b in ob) / n, 4),
                    mean_iter=round(sum(b["iter"] for b in ob) / n, 1),
                    worst_rel_gtop_large_vs_other=worst)
                print(json.dumps(rec), flush=True)
                if args.out:
                    os.makedirs(args.out, exist_ok=True)
                    fn = "batch_large_%s_%dx%d_n%d_vs_%s.json" % (name, args.m, args.n, n, args.against)
                    with open(os.path.join(args.out, fn), "w") as f:
                        json.dump(rec, f, indent=1)
                        f.write("\n")


if __name__ == "__main__":
    main()
