#!/usr/bin/env python3
"""What the clusters' geometry costs: the same items through
Context.batch_clusters (plain), through Context.batch_clusters(geometry=True)
and through the host loop the geometry call replaces (occupy / label(canon=
True) per item, then numpy sums over the sites), in one process on one GPU --
tools/cluster_bench.py's protocol.  Each item is its own trial at a fixed
point; the orders are drawn before the clock starts; a timed batch call
includes the rank arrays' upload and the read-back of everything it returns, a
timed loop every host call of its items and the numpy sums.  After one warm-up
of each the legs are timed alternately `repeats` times; the record keeps every
wall time, the best of each and the spreads.  The loop leg takes at most
--loop-cap items (its rate is per item).

  python tools/cluster_geometry_bench.py [--L 50,128 --items 1024 --repeats 5 --out DIR]
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
    ap.add_argument("--items", default="1024")
    ap.add_argument("--kinds", default="bond,site,mixed")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nexact", type=int, default=64)
    ap.add_argument("--loop-cap", type=int, default=128)
    ap.add_argument("--pb", type=float, default=0.5, help="bond case")
    ap.add_argument("--ps", type=float, default=0.6, help="site case")
    ap.add_argument("--mixed", default="0.90,0.65", help="mixed case: ps,pb")
    ap.add_argument("--out", default=None, help="directory for batch_geometry_<kind>_L<L>_n<items>.json")
    args = ap.parse_args()
    from percolation_amd import _lib as L
    from percolation_amd import api
    mps, mpb = (float(x) for x in args.mixed.split(","))
    sizes = [int(x) for x in args.items.split(",")]
    nmax = max(sizes)
    for Ls in (int(x) for x in args.L.split(",")):
        with api.Context(0, Ls, Ls, 0) as ctx:
            t, nb = ctx.t, ctx.nb
            x, y, wx, unit = api.site_positions(0, Ls, Ls)
            q = wx * x * x + y * y
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

                def batch(n, geometry):
                    return ctx.batch_clusters(kind, np.arange(n, dtype=np.int32),
                                              site_orders=None if so is None else so[:n],
                                              bond_orders=None if bo is None else bo[:n],
                                              item_nsites=None if so is None else np.full(n, ns, np.int32),
                                              item_nbonds=None if bo is None else np.full(n, nbc, np.int32),
                                              nexact=args.nexact, geometry=geometry)

                def loop(n):
                    """(n2, g2) per item from the canonical labels: a member
                    site has canon > 0 (bond kind: an end of an occupied bond)"""
                    out = []
                    for i in range(n):
                        ctx.occupy(kind, site_order=None if so is None else so[i], nsites=ns,
                                   bond_order=None if bo is None else bo[i], nbonds_=nbc)
                        lab = ctx.label(canon=True)["canon"].astype(np.int64)
                        sums = np.zeros((4, t + 1), dtype=np.int64)
                        for row, w in zip(sums, (1, q, x, y)):
                            np.add.at(row, lab, w)
                        sums[:, 0] = 0
                        nc, sq, sx, sy = sums
                        out.append((int((nc * nc).sum()), int((nc * sq - wx * sx * sx - sy * sy).sum())))
                    return out

                for n in sizes:
                    nl = min(n, args.loop_cap)
                    batch(n, False)  # warm-up of every leg at this size
                    batch(n, True)
                    loop(min(nl, 16))
                    wp, wg, wl = [], [], []
                    for _ in range(args.repeats):
                        t0 = time.perf_counter()
                        plain = batch(n, False)
                        wp.append(time.perf_counter() - t0)
                        t0 = time.perf_counter()
                        recs, hist, geom, rows = batch(n, True)
                        wg.append(time.perf_counter() - t0)
                        t0 = time.perf_counter()
                        ol = loop(nl)
                        wl.append(time.perf_counter() - t0)
                    bad = sum((int(g["n2"]), int(g["g2"])) != o for g, o in zip(geom, ol))
                    same = recs.tobytes() == plain[0].tobytes() and hist.tobytes() == plain[1].tobytes()
                    fin = (geom["n2"] - geom["span_n2"]).sum()
                    rec = dict(
                        workload="cluster_geometry_bench square %dx%d %s" % (Ls, Ls, name), kind=name, point=point,
                        items=n, nexact=args.nexact, repeats=args.repeats, loop_items=nl,
                        plain_wall_ms=[round(w * 1e3, 3) for w in wp],
                        geom_wall_ms=[round(w * 1e3, 3) for w in wg],
                        loop_wall_ms=[round(w * 1e3, 3) for w in wl],
                        plain_items_per_s=round(n / min(wp), 1), geom_items_per_s=round(n / min(wg), 1),
                        loop_items_per_s=round(nl / min(wl), 1),
                        geom_cost=round(min(wg) / min(wp) - 1, 4),
                        ratio_vs_loop=round((min(wl) / nl) / (min(wg) / n), 2),
                        plain_spread=round((max(wp) - min(wp)) / min(wp), 3),
                        geom_spread=round((max(wg) - min(wg)) / min(wg), 3),
                        loop_spread=round((max(wl) - min(wl)) / min(wl), 3),
                        loop_mismatches=int(bad), records_equal_plain=bool(same),
                        xi=round(float(np.sqrt(2.0 * (geom["g2"] - geom["span_g2"]).sum() / (unit * fin))), 4)
                        if fin else None,
                        mean_big_n=round(float(geom["big_n"].mean()), 1))
                    print(json.dumps(rec), flush=True)
                    if args.out:
                        os.makedirs(args.out, exist_ok=True)
                        fn = "batch_geometry_%s_L%d_n%d.json" % (name, Ls, n)
                        with open(os.path.join(args.out, fn), "w") as f:
                            json.dump(rec, f, indent=1)
                            f.write("\n")


if __name__ == "__main__":
    main()
