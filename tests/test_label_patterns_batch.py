"""The one-workgroup kernels (k_batch_cond, k_batch_scan; lds_label of
perc_batch_uf.h: "hook, flatten, until nothing changed") on the structured
occupancies of label_patterns.py: chains as long as the lattice, stripes with
up to m / 2 spanning clusters, combs -- against the single path
(perc_label, perc_first_spanning, perc_cluster_sizes) and the oracle.  The
orders and the oracle's first spanning counts are pinned on the CPU by
test_label_patterns_host.py.
"""
import numpy as np
import pytest

import label_patterns as LP
from percolation_amd import _lib as PL
from percolation_amd import api
from test_label_patterns import occupy
from test_label_patterns_host import BATCH_COND, BATCH_SCAN, KIND, nclusters, scan_cases

pytestmark = pytest.mark.gpu
LABEL_KEYS = ("nclusters", "nspan", "span_root", "span_sites")
NOTHING_SPANS = {"bond": ("serp_short", "combs"), "site": ("serp_short", "combs"),
                 "mixed": ("s:serp_short", "s:combs", "b:serp_short", "b:combs")}


def batch_kw(kind_name, so_rows, bo_rows, ns, nbc):
    kw = {}
    if kind_name != "bond":
        kw.update(site_orders=np.stack(so_rows), item_nsites=np.array(ns, np.int32))
    if kind_name != "site":
        kw.update(bond_orders=np.stack(bo_rows), item_nbonds=np.array(nbc, np.int32))
    return kw


@pytest.mark.parametrize("geom", BATCH_COND)
@pytest.mark.parametrize("kind_name", LP.KINDS)
def test_batch_cond_labels_of_patterns(geom, kind_name):
    lat, m, n, pbc = geom
    assert api.batch_cond_supported(KIND[kind_name], lat, m, n, pbc)
    t, nb = m * n, api.nbonds(lat, m, n, pbc)
    cases = LP.cases(kind_name, lat, m, n, pbc)
    # every pattern twice, at different places of the batch
    seq = list(range(len(cases))) + list(range(len(cases)))[::-1]
    ref = []
    with api.Context(lat, m, n, pbc) as ctx:
        for i, (name, sids, bids) in enumerate(cases):
            order = LP.ORDERS[i % 3]
            so = None if sids is None else LP.ordered(sids, order, 300 + i)
            bo = None if bids is None else LP.ordered(bids, order, 400 + i)
            on = LP.oracle_numbers(kind_name, lat, m, n, pbc, so, bo)
            roots = LP.spanning_roots(on["canon"], m, n)
            w = dict(nclusters=nclusters(on["canon"]), nspan=len(roots), span_root=on["span_root"],
                     span_sites=int(np.count_nonzero(on["canon"] == on["span_root"])) if len(roots) else 0)
            occupy(ctx, kind_name, so, bo)
            li = ctx.label()
            for k in LABEL_KEYS:  # the single path equals the oracle
                assert li[k] == w[k], (name, order, k, li[k], w[k])
            ref.append((w, "%s (%s order)" % (name, order), so, bo))
        so_rows, bo_rows, ns, nbc, want, names = [], [], [], [], [], []
        for i in seq:
            w, tag, so, bo = ref[i]
            want.append(w)
            names.append(tag)
            if so is not None:
                so_rows.append(LP.order_row(so, t))
                ns.append(len(so))
            if bo is not None:
                bo_rows.append(LP.order_row(bo, nb))
                nbc.append(len(bo))
        kw = batch_kw(kind_name, so_rows, bo_rows, ns, nbc)
        out = ctx.batch_cond(KIND[kind_name], np.arange(len(seq), dtype=np.int32), solve=False, **kw)
        assert len(out) == len(seq)
        for j, (o, w) in enumerate(zip(out, want)):
            for k in LABEL_KEYS:
                assert o[k] == w[k], (names[j], j, k, o[k], w[k])
            assert o["fallback"] == (1 if w["nspan"] > 1 else 0), (names[j], j, o)
        for j in range(len(cases)):  # the two copies of a pattern
            assert repr(out[j]) == repr(out[len(seq) - 1 - j]), (names[j], out[j], out[len(seq) - 1 - j])
        assert {min(w["nspan"], 2) for w in want} == {0, 1, 2}
        # nothing spans: the solve has nothing to do
        pick = [j for j in range(len(cases)) if cases[j][0] in NOTHING_SPANS[kind_name]]
        assert len(pick) == len(NOTHING_SPANS[kind_name])
        sub = {k: (v[pick] if v.ndim == 1 else v) for k, v in kw.items()}
        out = ctx.batch_cond(KIND[kind_name], np.array(pick, np.int32), solve=True, **sub)
        for j, o in zip(pick, out):
            assert want[j]["nspan"] == 0, names[j]
            assert o["status"] == 1 and o["gtop"] == 0.0 and o["gbot"] == 0.0, (names[j], o)
            assert o["nspan"] == 0 and o["nclusters"] == want[j]["nclusters"], (names[j], o)


@pytest.mark.parametrize("geom", BATCH_SCAN)
def test_batch_scan_of_patterns(geom):
    lat, m, n, pbc = geom
    assert api.scan_supported(lat, m, n, pbc)
    sc = scan_cases(geom)
    with api.Context(lat, m, n, pbc) as ctx:
        for kind in (PL.BOND, PL.SITE):
            cs = [c for c in sc if c["kind"] == kind]
            assert len(cs) == 2
            key = "bond_orders" if kind == PL.BOND else "site_orders"
            rows = np.stack([c["bo"] if kind == PL.BOND else c["so"] for c in cs])
            got = ctx.batch_scan(kind, **{key: rows})
            for c, g, row in zip(cs, got, rows):
                assert g["first"] == c["first"], (c["name"], g, c["first"])  # the oracle's bisection
                first = api.first_spanning(ctx, row, kind)  # the single path
                assert g["first"] == first, (c["name"], g, first)
                assert (g["maxcs"], g["span_size"]) == ctx.cluster_sizes(), (c["name"], g, ctx.cluster_sizes())
                assert g["nspan"] == 1, (c["name"], g)
            assert got[0]["first"] == cs[0]["length"], (cs[0]["name"], got[0])  # with the final element
        for c in sc:
            if c["kind"] != PL.SITEBOND:
                continue
            g = ctx.batch_scan(PL.SITEBOND, site_orders=c["so"], bond_orders=c["bo"], scan=c["scan"],
                               fixed=c["fixed"])[0]
            assert g["first"] == c["first"], (c["name"], g, c["first"])
            t, nb = ctx.t, ctx.nb
            if c["scan"] == PL.BOND:
                first = api.first_spanning_mixed(ctx, PL.BOND, c["so"], c["fixed"], c["bo"], nb)
            else:
                first = api.first_spanning_mixed(ctx, PL.SITE, c["so"], t, c["bo"], c["fixed"])
            assert g["first"] == first, (c["name"], g, first)
            assert g["nspan"] == 1 and (g["maxcs"], g["span_size"]) == (0, 0), (c["name"], g)
