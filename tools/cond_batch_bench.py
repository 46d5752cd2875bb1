#!/usr/bin/env python3
"""Site and mixed conductance items through Context.batch_cond (one workgroup
per item, one launch) and through the single-path loop (occupy / label /
conductance per item), the same items, in one process on one GPU: items/s of
both and their ratio.  Each item is its own trial (its own shuffled orders) at
a fixed point: site at ps, mixed at (ps, pb).  The orders are drawn before the
clock starts; a timed batch call includes the rank arrays' upload and the read-
back, a timed loop every host call of its items.  After one warm-up of each the
two are timed alternately `repeats` times; the record keeps every wall time,
the best of each and the spread.

  python tools/cond_batch_bench.py [--L 50 --items 256,1024 --repeats 5 --out DIR]
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
    ap.add_argument("--L", type=int, default=50)
    ap.add_argument("--items", default="256,1024")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ps", type=float, default=0.66, help="site case")
    ap.add_argument("--mixed", default="0.90,0.80", help="mixed case: ps,pb")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--itmax", type=int, default=2500)
    ap.add_argument("--literal", action="store_true")
    ap.add_argument("--out", default=None, help="directory for batch_cond_<kind>_L<L>_n<items>.json")
    args = ap.parse_args()
    from percolation_amd import _lib as L
    from percolation_amd import api
    mps, mpb = (float(x) for x in args.mixed.split(","))
    sizes = [int(x) for x in args.items.split(",")]
    nmax = max(sizes)
    with api.Context(0, args.L, args.L, 0) as ctx:
        if args.literal:
            ctx.set_dot_order(L.DOT_LITERAL)
        t, nb = ctx.t, ctx.nb
        tseed = api.trial_seeds(58302, nmax)
        sseed, bseed = api.paired_seeds(8811064, nmax)
        cases = [
            ("site", L.SITE, dict(ps=args.ps), int(args.ps * t), 0,
             np.stack([api.shuffled_ids(t, int(s)) for s in tseed]), None),
            ("mixed", L.SITEBOND, dict(ps=mps, pb=mpb), int(mps * t), int(mpb * nb),
             np.stack([api.shuffled_ids(t, int(s)) for s in sseed]),
             np.stack([api.shuffled_ids(nb, int(s)) for s in bseed])),
        ]
        for name, kind, point, ns, nbc, so, bo in cases:
            rule, cur = api.KIND_RULE[kind], api.natural_cur_rule(kind)

            def batch(n):
                return ctx.batch_cond(kind, np.arange(n, dtype=np.int32), site_orders=so[:n],
                                      bond_orders=None if bo is None else bo[:n],
                                      item_nsites=np.full(n, ns, np.int32),
                                      item_nbonds=None if bo is None else np.full(n, nbc, np.int32),
                                      tol=args.tol, itmax=args.itmax)

            def loop(n):
                out = []
                for i in range(n):
                    if bo is None:
                        ctx.occupy(kind, site_order=so[i], nsites=ns)
                    else:
                        ctx.occupy(kind, site_order=so[i], nsites=ns, bond_order=bo[i], nbonds_=nbc)
                    li = ctx.label()
                    c = ctx.conductance(rule, cur, 1.0, 1.0, api.LEAK, 2, args.tol, args.itmax)
                    out.append((li["nspan"], c["gtop"], c["iter"]))
                return out

            for n in sizes:
                batch(n)  # warm-up of both paths at this size
                loop(min(n, 64))
                wb, wl = [], []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    ob = batch(n)
                    wb.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    ol = loop(n)
                    wl.append(time.perf_counter() - t0)
                # the two paths solved the same items (each in its own fast
                # association: the distance of the two Gtop is recorded)
                worst = 0.0
                for b, (nspan, gtop, _) in zip(ob, ol):
                    assert b["nspan"] == nspan, (b, nspan)
                    if gtop:
                        worst = max(worst, abs(b["gtop"] - gtop) / abs(gtop))
                rec = dict(
                    workload="cond_batch_bench square L=%d %s" % (args.L, name), kind=name, point=point,
                    items=n, dot="literal" if args.literal else "fast", tol=args.tol, repeats=args.repeats,
                    batch_wall_ms=[round(w * 1e3, 3) for w in wb],
                    loop_wall_ms=[round(w * 1e3, 3) for w in wl],
                    batch_items_per_s=round(n / min(wb), 1), loop_items_per_s=round(n / min(wl), 1),
                    ratio=round(min(wl) / min(wb), 2),
                    ratio_median=round(float(np.median(wl) / np.median(wb)), 2),
                    batch_spread=round((max(wb) - min(wb)) / min(wb), 3),
                    loop_spread=round((max(wl) - min(wl)) / min(wl), 3),
                    spanning_share=round(sum(b["nspan"] > 0 for b in ob) / n, 4),
                    fallback_share=round(sum(b["fallback"] for b in ob) / n, 4),
                    mean_iter=round(sum(b["iter"] for b in ob) / n, 1),
                    worst_rel_gtop_batch_vs_loop=worst)
                print(json.dumps(rec), flush=True)
                if args.out:
                    os.makedirs(args.out, exist_ok=True)
                    with open(os.path.join(args.out, "batch_cond_%s_L%d_n%d.json" % (name, args.L, n)), "w") as f:
                        json.dump(rec, f, indent=1)
                        f.write("\n")


if __name__ == "__main__":
    main()
