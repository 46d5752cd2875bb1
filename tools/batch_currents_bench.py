#!/usr/bin/env python3
"""What the bond-current record costs and what it saves, on the same items in
one process on one GPU (cond_batch_bench's protocol):

  (a) Context.batch_cond(currents=True) against the unchanged batch_cond: the
      cost of the epilogue, the record's read-back and its Python dicts;
  (b) Context.batch_cond(currents=True) against the single-path loop a user
      runs without it: occupy / label(canon) / conductance(vint=True) per item,
      then conducting_bonds and current_stats_host.

Each item is its own trial at a fixed point: bond at pb, site at ps, mixed at
(ps, pb).  The orders are drawn before the clock starts; a timed batch call
includes the rank arrays' upload and the read-back, a timed loop every host
call of its items.  After one warm-up of each the three are timed alternately
`repeats` times; the record keeps every wall time, the best of each, both
ratios and the spreads.

  python tools/batch_currents_bench.py [--L 50 --items 256,1024 --repeats 5 --out DIR]
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
    ap.add_argument("--pb", type=float, default=0.60, help="bond case")
    ap.add_argument("--ps", type=float, default=0.66, help="site case")
    ap.add_argument("--mixed", default="0.90,0.80", help="mixed case: ps,pb")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--itmax", type=int, default=2500)
    ap.add_argument("--cut", type=float, default=1e-6)
    ap.add_argument("--literal", action="store_true")
    ap.add_argument("--out", default=None, help="directory for batch_currents_<kind>_L<L>_n<items>.json")
    args = ap.parse_args()
    from percolation_amd import _lib as L
    from percolation_amd import api
    mps, mpb = (float(x) for x in args.mixed.split(","))
    sizes = [int(x) for x in args.items.split(",")]
    nmax = max(sizes)
    lat = (0, args.L, args.L, 0)
    with api.Context(*lat) as ctx:
        if args.literal:
            ctx.set_dot_order(L.DOT_LITERAL)
        t, nb = ctx.t, ctx.nb
        b1, b2 = api.bond_list(*lat)
        tseed = api.trial_seeds(58302, nmax)
        sseed, bseed = api.paired_seeds(8811064, nmax)
        cases = [
            ("bond", L.BOND, dict(pb=args.pb), 0, int(args.pb * nb), None,
             np.stack([api.shuffled_ids(nb, int(s)) for s in tseed])),
            ("site", L.SITE, dict(ps=args.ps), int(args.ps * t), 0,
             np.stack([api.shuffled_ids(t, int(s)) for s in tseed]), None),
            ("mixed", L.SITEBOND, dict(ps=mps, pb=mpb), int(mps * t), int(mpb * nb),
             np.stack([api.shuffled_ids(t, int(s)) for s in sseed]),
             np.stack([api.shuffled_ids(nb, int(s)) for s in bseed])),
        ]
        for name, kind, point, ns, nbc, so, bo in cases:
            rule, cur = api.KIND_RULE[kind], api.natural_cur_rule(kind)

            def batch(n, **kw):
                return ctx.batch_cond(kind, np.arange(n, dtype=np.int32),
                                      site_orders=None if so is None else so[:n],
                                      bond_orders=None if bo is None else bo[:n],
                                      item_nsites=None if so is None else np.full(n, ns, np.int32),
                                      item_nbonds=None if bo is None else np.full(n, nbc, np.int32),
                                      tol=args.tol, itmax=args.itmax, **kw)

            def loop(n):
                out = []
                for i in range(n):
                    ctx.occupy(kind, site_order=None if so is None else so[i], nsites=ns,
                               bond_order=None if bo is None else bo[i], nbonds_=nbc)
                    li = ctx.label(canon=True)
                    c = ctx.conductance(rule, cur, 1.0, 1.0, api.LEAK, 2, args.tol, args.itmax, vint=True)
                    socc, bocc = ctx.occupancy()
                    mask = api.conducting_bonds(kind, b1, b2, socc, bocc, li["canon"], li["span_root"])
                    out.append((li["nspan"], c["gtop"],
                                api.current_stats_host(*lat, mask, c["vint"], 1.0, 1.0, args.cut)))
                return out

            for n in sizes:
                batch(n, currents=True, cut=args.cut)  # warm-up of the three paths at this size
                batch(n)
                loop(min(n, 64))
                wc, wp, wl = [], [], []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    oc = batch(n, currents=True, cut=args.cut)
                    wc.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    op = batch(n)
                    wp.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    ol = loop(n)
                    wl.append(time.perf_counter() - t0)
                # the three paths solved the same items: batch_cond's record
                # unchanged, the loop's counts those of the batch (each in its own
                # fast association: the distance of the two s2 is recorded)
                worst = 0.0
                for c, p, (nspan, gtop, r) in zip(oc, op, ol):
                    assert all(c[k] == p[k] for k in p), (c, p)
                    assert c["nspan"] == nspan, (c, nspan)
                    if c["fallback"] == 0 and c["status"] == 0:
                        assert c["nbonds"] == r["nbonds"], (c, r)
                        worst = max(worst, abs(c["s2"] - r["s2"]) / abs(r["s2"]))
                span = [c for c in oc if c["nbonds"]]
                rec = dict(
                    workload="batch_currents_bench square L=%d %s" % (args.L, name), kind=name, point=point,
                    items=n, dot="literal" if args.literal else "fast", tol=args.tol, cut=args.cut,
                    repeats=args.repeats,
                    currents_wall_ms=[round(w * 1e3, 3) for w in wc],
                    plain_wall_ms=[round(w * 1e3, 3) for w in wp],
                    loop_wall_ms=[round(w * 1e3, 3) for w in wl],
                    currents_items_per_s=round(n / min(wc), 1), plain_items_per_s=round(n / min(wp), 1),
                    loop_items_per_s=round(n / min(wl), 1),
                    epilogue_cost=round(min(wc) / min(wp), 3),
                    epilogue_cost_median=round(float(np.median(wc) / np.median(wp)), 3),
                    ratio_vs_loop=round(min(wl) / min(wc), 2),
                    ratio_vs_loop_median=round(float(np.median(wl) / np.median(wc)), 2),
                    currents_spread=round((max(wc) - min(wc)) / min(wc), 3),
                    plain_spread=round((max(wp) - min(wp)) / min(wp), 3),
                    loop_spread=round((max(wl) - min(wl)) / min(wl), 3),
                    spanning_share=round(sum(c["nspan"] > 0 for c in oc) / n, 4),
                    fallback_share=round(sum(c["fallback"] for c in oc) / n, 4),
                    mean_iter=round(sum(c["iter"] for c in oc) / n, 1),
                    mean_backbone=round(float(np.mean([c["nabove"] / c["nbonds"] for c in span])), 4) if span else 0.0,
                    worst_rel_s2_batch_vs_loop=worst)
                print(json.dumps(rec), flush=True)
                if args.out:
                    os.makedirs(args.out, exist_ok=True)
                    with open(os.path.join(args.out, "batch_currents_%s_L%d_n%d.json" % (name, args.L, n)), "w") as f:
                        json.dump(rec, f, indent=1)
                        f.write("\n")


if __name__ == "__main__":
    main()
