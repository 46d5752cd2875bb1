#!/usr/bin/env python3
"""Conductance with random bond weights (ConductCalc condtype 2) through
Context.batch_cond(item_wseed=..) -- k_twister_stream and k_batch_cond_w, one
workgroup per item, one launch -- and through the single path's own weighted
loop (occupy / label / set_conductcalc_weights / conductance per item), the
same items and seeds, in one process on one GPU: items/s of both and their
ratio.  The unweighted perc_batch_cond runs on the same items as well: what
the stored values, the draws and the weight rows cost beside the two-value
codes.  Each item is its own trial (its own shuffled orders) at a fixed point:
bond at pb, site at ps, mixed at (ps, pb); item i draws with seed wseed + i.
The orders are drawn before the clock starts; a timed batch call includes the
rank arrays' upload and the read-back, a timed loop every host call of its
items.  After one warm-up of each the three are timed alternately `repeats`
times; the record keeps every wall time, the best of each and the spread.

  python tools/batch_weighted_bench.py [--L 50 --items 256,1024 --repeats 5 --out DIR]
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
    ap.add_argument("--lattice", type=int, default=0)
    ap.add_argument("--pbc", type=int, default=0)
    ap.add_argument("--items", default="256,1024")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pb", type=float, default=0.60, help="bond case")
    ap.add_argument("--ps", type=float, default=0.66, help="site case")
    ap.add_argument("--mixed", default="0.90,0.80", help="mixed case: ps,pb")
    ap.add_argument("--kinds", default="bond,site,mixed")
    ap.add_argument("--wseed", type=int, default=1838534)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--itmax", type=int, default=2500)
    ap.add_argument("--literal", action="store_true")
    ap.add_argument("--out", default=None, help="directory for batch_weighted_<kind>_L<L>_n<items>.json")
    args = ap.parse_args()
    from percolation_amd import _lib as L
    from percolation_amd import api
    mps, mpb = (float(x) for x in args.mixed.split(","))
    sizes = [int(x) for x in args.items.split(",")]
    nmax = max(sizes)
    lat = (args.lattice, args.L, args.L, args.pbc)
    with api.Context(*lat) as ctx:
        if args.literal:
            ctx.set_dot_order(L.DOT_LITERAL)
        t, nb = ctx.t, ctx.nb
        tseed = api.trial_seeds(58302, nmax)
        sseed, bseed = api.paired_seeds(8811064, nmax)
        site_o = np.stack([api.shuffled_ids(t, int(s)) for s in tseed])
        bond_o = np.stack([api.shuffled_ids(nb, int(s)) for s in tseed])
        cases = [
            ("bond", L.BOND, dict(pb=args.pb), 0, int(args.pb * nb), None, bond_o),
            ("site", L.SITE, dict(ps=args.ps), int(args.ps * t), 0, site_o, None),
            ("mixed", L.SITEBOND, dict(ps=mps, pb=mpb), int(mps * t), int(mpb * nb),
             np.stack([api.shuffled_ids(t, int(s)) for s in sseed]),
             np.stack([api.shuffled_ids(nb, int(s)) for s in bseed])),
        ]
        for name, kind, point, ns, nbc, so, bo in cases:
            if name not in args.kinds.split(","):
                continue
            assert api.batch_weighted_supported(kind, *lat), lat
            rule, cur = api.KIND_RULE[kind], api.natural_cur_rule(kind)

            def batch(n, weighted=True):
                kw = dict(item_wseed=args.wseed + np.arange(n, dtype=np.int64)) if weighted else {}
                return ctx.batch_cond(kind, np.arange(n, dtype=np.int32), site_orders=None if so is None else so[:n],
                                      bond_orders=None if bo is None else bo[:n],
                                      item_nsites=None if so is None else np.full(n, ns, np.int32),
                                      item_nbonds=None if bo is None else np.full(n, nbc, np.int32),
                                      tol=args.tol, itmax=args.itmax, **kw)

            def loop(n):
                out = []
                for i in range(n):
                    if so is None:
                        ctx.occupy(kind, bond_order=bo[i], nbonds_=nbc)
                    elif bo is None:
                        ctx.occupy(kind, site_order=so[i], nsites=ns)
                    else:
                        ctx.occupy(kind, site_order=so[i], nsites=ns, bond_order=bo[i], nbonds_=nbc)
                    li = ctx.label()
                    ctx.set_conductcalc_weights(rule, args.wseed + i)
                    c = ctx.conductance(rule, cur, 1.0, 1.0, api.LEAK, 2, args.tol, args.itmax)
                    out.append((li["nspan"], c["gtop"], c["iter"]))
                ctx.set_bond_weights(None)
                return out

            for n in sizes:
                batch(n)  # warm-up of the three paths at this size
                batch(n, False)
                loop(min(n, 64))
                ww, wu, wl = [], [], []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    ob = batch(n)
                    ww.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    ou = batch(n, False)
                    wu.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    ol = loop(n)
                    wl.append(time.perf_counter() - t0)
                # the two weighted paths solved the same items (each in its
                # own fast association: the distance of the two Gtop is recorded)
                worst = 0.0
                for b, (nspan, gtop, _) in zip(ob, ol):
                    assert b["nspan"] == nspan, (b, nspan)
                    if gtop:
                        worst = max(worst, abs(b["gtop"] - gtop) / abs(gtop))
                rec = dict(
                    workload="batch_weighted_bench %s L=%d %s%s" % ("triangular" if args.lattice else "square", args.L,
                                                                   name, " pbc" if args.pbc else ""),
                    kind=name, point=point, items=n, dot="literal" if args.literal else "fast", tol=args.tol,
                    repeats=args.repeats, mode="ConductCalc seeds",
                    weighted_batch_wall_ms=[round(w * 1e3, 3) for w in ww],
                    unweighted_batch_wall_ms=[round(w * 1e3, 3) for w in wu],
                    weighted_loop_wall_ms=[round(w * 1e3, 3) for w in wl],
                    weighted_batch_items_per_s=round(n / min(ww), 1),
                    unweighted_batch_items_per_s=round(n / min(wu), 1),
                    weighted_loop_items_per_s=round(n / min(wl), 1),
                    ratio_vs_loop=round(min(wl) / min(ww), 2),
                    ratio_vs_loop_median=round(float(np.median(wl) / np.median(ww)), 2),
                    ratio_vs_unweighted_batch=round(min(wu) / min(ww), 3),
                    weighted_batch_spread=round((max(ww) - min(ww)) / min(ww), 3),
                    unweighted_batch_spread=round((max(wu) - min(wu)) / min(wu), 3),
                    loop_spread=round((max(wl) - min(wl)) / min(wl), 3),
                    spanning_share=round(sum(b["nspan"] > 0 for b in ob) / n, 4),
                    fallback_share=round(sum(b["fallback"] for b in ob) / n, 4),
                    mean_iter_weighted=round(sum(b["iter"] for b in ob) / n, 1),
                    mean_iter_unweighted=round(sum(b["iter"] for b in ou) / n, 1),
                    worst_rel_gtop_batch_vs_loop=worst)
                print(json.dumps(rec), flush=True)
                if args.out:
                    os.makedirs(args.out, exist_ok=True)
                    with open(os.path.join(args.out, "batch_weighted_%s_L%d_n%d.json" % (name, args.L, n)), "w") as f:
                        json.dump(rec, f, indent=1)
                        f.write("\n")


if __name__ == "__main__":
    main()
