"""The batch path for site and mixed conductance (perc_batch_cond,
k_batch_cond): many small realisations of any kind in one launch, one
workgroup each, checked against the single path (perc_occupy / perc_label /
perc_conductance) item by item:

* labels and the outcomes (nothing spans, one cluster, several -> fallback)
  on a grid of counts of three trials per lattice, site and mixed kinds;
* the literal dot order bitwise (conductances, iterations, err) under both
  current rules; the bond kind dict for dict perc_batch_bondc's;
* the oracle's linbcg and currents on the four small rule_systems systems,
  unit and non-unit values (the leak on both sides of the 1e-10 threshold);
* the fast order: deterministic, independent of the item's place in the
  grid, as accurate as test_batch.check_accuracy asks;
* the size cap (N = 8192), a ragged last thread row (N = 8190), the largest
  labeling view (triangular 64 x 130 pbc), the spill slot, a forced
  two-cluster fallback, every PERC_EINVAL case, and api.cond_curve batched
  against unbatched.

The single-path reference of a (lattice, kind) is computed once and shared."""
import ctypes as C

import numpy as np
import pytest

import rule_systems as R
import test_batch as TB
from percolation_amd import _lib as L
from percolation_amd import api

pytestmark = pytest.mark.gpu
TOL, ITMAX = 1e-8, 2500
TIGHT, TIGHT_ITMAX = 1e-13, 20000
LATTICES = [(0, 10, 10, 0), (0, 10, 10, 1), (1, 10, 10, 0), (1, 12, 10, 1), (0, 50, 50, 0)]
KINDS = [L.SITE, L.SITEBOND]
KIND_NAME = {L.SITE: "site", L.SITEBOND: "mixed"}
CURS = [L.CUR_FORTRAN, L.CUR_MATLAB]
LABEL_KEYS = ("nclusters", "nspan", "span_root", "span_sites")
COND_KEYS = ("gtop", "gbot", "iter", "err", "status")


def prefix(order, count, N):
    """perc_occupy's arguments for the first `count` entries of an order of
    N + 1 (N + 1: the whole order, the spill slot dropped)"""
    if count > N:
        o = np.ascontiguousarray(order[order != 0])
        return o, len(o)
    return order, int(count)


def occupy(ctx, kind, so, ns, bo=None, nbc=0):
    if kind == L.SITE:
        o, k = prefix(so, ns, ctx.t)
        ctx.occupy(L.SITE, site_order=o, nsites=k)
    else:
        o, k = prefix(so, ns, ctx.t)
        b, kb = prefix(bo, nbc, ctx.nb)
        ctx.occupy(L.SITEBOND, site_order=o, nsites=k, bond_order=b, nbonds_=kb)


def single(ctx, kind, so, ns, bo=None, nbc=0, solve=True, tol=TOL, itmax=ITMAX, Va=1.0, g0=1.0,
           leak=api.LEAK):
    """the single path on one item: the labels and, per current rule, the
    conductance record (one solve; the second rule's currents of the same
    voltages by perc_currents, as perc_conductance forms them)"""
    occupy(ctx, kind, so, ns, bo, nbc)
    li = ctx.label()
    if not solve:
        return li, None
    rule = api.KIND_RULE[kind]
    c = ctx.conductance(rule, L.CUR_MATLAB, Va, g0, leak, 2, tol, itmax)
    cond = {L.CUR_MATLAB: c}
    f = dict(c)
    if c["status"] == 0:
        res = L.CondResult()
        L.check(L.lib().perc_currents(ctx.h, rule, L.CUR_FORTRAN, Va, g0, leak, C.byref(res)), "perc_currents")
        f["gtop"], f["gbot"] = res.gtop, res.gbot
    cond[L.CUR_FORTRAN] = f
    return li, cond


def items_of(kind, lat):
    """(seeds, items): items (trial, nsites, nbonds) of the issue's grids"""
    lattice, m, n, pbc = lat
    t, nb = m * n, api.nbonds(*lat)
    if kind == L.SITE:
        seeds = (api.trial_seeds(58302, 3), None)
        counts = sorted({int(round(0.05 * k * t)) for k in range(1, 21)} | {0, 1, t, t + 1})
        return seeds, [(tr, c, 0) for tr in range(3) for c in counts]
    seeds = (api.trial_seeds(143285, 3), api.trial_seeds(43716, 3))
    return seeds, [(tr, int(round(ps * t)), int(round(pb * nb))) for tr in range(3) for ps in (0.8, 0.9, 1.0)
                   for pb in (0.5, 0.6, 0.7, 0.8, 0.9, 1.0)]


_REF = {}


def reference(lat, kind):
    """orders, items and the single path's labels and literal conductances
    (tol 1e-8, itmax 2500, both current rules), computed once"""
    if (lat, kind) in _REF:
        return _REF[lat, kind]
    (ss, bs), it = items_of(kind, lat)
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        so = np.stack([api.shuffled_ids(ctx.t, int(s)) for s in ss])
        bo = np.stack([api.shuffled_ids(ctx.nb, int(s)) for s in bs]) if bs is not None else None
        lab, cond = [], []
        for tr, ns, nbc in it:
            li, c = single(ctx, kind, so[tr], ns, None if bo is None else bo[tr], nbc)
            lab.append(li)
            cond.append(c)
    _REF[lat, kind] = dict(so=so, bo=bo, trial=np.array([x[0] for x in it], np.int32),
                           ns=np.array([x[1] for x in it], np.int32),
                           nb=np.array([x[2] for x in it], np.int32) if bo is not None else None,
                           label=lab, cond=cond)
    return _REF[lat, kind]


def run(ctx, kind, ref, **kw):
    return ctx.batch_cond(kind, ref["trial"], site_orders=ref["so"], bond_orders=ref["bo"],
                          item_nsites=ref["ns"], item_nbonds=ref["nb"], **kw)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_NAME.get)
@pytest.mark.parametrize("lat", LATTICES)
def test_labels_and_outcomes(lat, kind):
    ref = reference(lat, kind)
    assert len(ref["label"]) == (69 if kind == L.SITE else 54)
    with api.Context(*lat) as ctx:
        out = run(ctx, kind, ref, solve=False)
    assert len(out) == len(ref["label"])
    seen = set()
    for i, (o, li) in enumerate(zip(out, ref["label"])):
        for k in LABEL_KEYS:
            assert o[k] == li[k], (k, i, int(ref["trial"][i]), int(ref["ns"][i]), o, li)
        assert o["fallback"] == (1 if li["nspan"] > 1 else 0), (i, o, li)
        seen.add(min(li["nspan"], 2))
    # a batch that falls back everywhere must not pass: the share of items
    # several clusters span, on the single path's own count
    multi = sum(li["nspan"] > 1 for li in ref["label"])
    once = sum(li["nspan"] == 1 for li in ref["label"])
    print("lattice %s %s: %d / %d items span once, %d with nspan > 1"
          % (lat, KIND_NAME[kind], once, len(out), multi))
    assert multi <= 0.10 * len(out)
    assert {0, 1} <= seen  # nothing spans and one cluster spans both occur


@pytest.mark.parametrize("cur", CURS, ids=["fortran", "matlab"])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_NAME.get)
@pytest.mark.parametrize("lat", LATTICES)
def test_literal_order_bitwise(lat, kind, cur):
    ref = reference(lat, kind)
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        out = run(ctx, kind, ref, cur_rule=cur, tol=TOL, itmax=ITMAX)
    solved = 0
    for i, (o, c) in enumerate(zip(out, ref["cond"])):
        for k in COND_KEYS:
            assert o[k] == c[cur][k], (k, i, int(ref["trial"][i]), int(ref["ns"][i]), o, c[cur])
        solved += o["status"] == 0 and o["iter"] > 0
    assert solved > 0


def test_default_rules_are_the_reference_pairing():
    lat, kind = (0, 10, 10, 0), L.SITE
    ref = reference(lat, kind)
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        a = run(ctx, kind, ref)
        b = run(ctx, kind, ref, rule=L.RULE_SITE, cur_rule=L.CUR_MATLAB)
    assert a == b


@pytest.mark.parametrize("order", [L.DOT_LITERAL, L.DOT_FAST], ids=["literal", "fast"])
def test_bond_kind_unchanged(order):
    ref = TB.reference((0, 50, 50, 0))
    with api.Context(0, 50, 50, 0) as ctx:
        ctx.set_dot_order(order)
        want = ctx.batch_bondc(ref["orders"], ref["trial"], ref["count"], tol=TOL, itmax=ITMAX)
        got = ctx.batch_cond(L.BOND, ref["trial"], bond_orders=ref["orders"], item_nbonds=ref["count"],
                             tol=TOL, itmax=ITMAX)
    assert len(got) == len(want) > 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
    assert any(w["status"] == 0 and w["iter"] > 0 for w in want)


def one_item(ctx, s, occ, cur, tol):
    kind = occ["kind"]
    return ctx.batch_cond(kind, [0], site_orders=occ["site_order"], bond_orders=occ.get("bond_order"),
                          item_nsites=[occ["nsites"]],
                          item_nbonds=[occ["nbonds_"]] if kind == L.SITEBOND else None,
                          rule=s.rule, cur_rule=cur, Va=s.Va, g0=s.g0, leak=s.leak, tol=tol, itmax=R.ITMAX)[0]


ORACLE_SYSTEMS = ([R.System(rule, *g, *R.UNIT) for rule in (L.RULE_SITE, L.RULE_MIXED)
                   for g in (R.G_SMALL_SQ, R.G_SMALL_TRI)]
                  + [R.System(rule, *R.G_SMALL_SQ, *v) for rule in (L.RULE_SITE, L.RULE_MIXED)
                     for v in R.NONUNIT])


@pytest.mark.parametrize("s", ORACLE_SYSTEMS, ids=R.name)
def test_oracle_linbcg_and_currents_bitwise(s):
    """one batch item per system in the literal order at both tols: iter and
    err the oracle's linbcg's, Gtop and Gbot its currents under both rules
    (non-unit values: the leak below and above the 1e-10 threshold, the
    Fortran rule's drop and keep branches)"""
    d = R.build(s)
    assert d["nspan"] == 1
    with api.Context(*R.geometry(s)) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        for tol in R.TOLS:
            oc = R.oracle_solve(s, tol)
            for cur in CURS:
                o = one_item(ctx, s, d["occ"], cur, tol)
                assert o["nspan"] == 1 and o["fallback"] == 0 and o["status"] == 0
                assert o["iter"] == oc["iter"] and o["err"] == oc["err"], (tol, cur, o, oc["iter"], oc["err"])
                assert (o["gtop"], o["gbot"]) == oc["cur"][cur], (tol, cur, o, oc["cur"][cur])


def fast_grid(ref):
    """300 items of the 50 x 50 site reference, the same item first and last"""
    t = 2500
    probe = (0, int(round(0.70 * t)))
    grid = [int(c) for c in sorted(set(ref["ns"].tolist())) if 0 < c <= t]
    items = [probe] + [(i % 3, grid[(7 * i) % len(grid)]) for i in range(1, 299)] + [probe]
    assert len(items) == 300
    return np.array([x[0] for x in items], np.int32), np.array([x[1] for x in items], np.int32)


def test_fast_order_deterministic_and_position_independent():
    lat = (0, 50, 50, 0)
    ref = reference(lat, L.SITE)
    it, ns = fast_grid(ref)
    with api.Context(*lat) as ctx:
        a = ctx.batch_cond(L.SITE, it, site_orders=ref["so"], item_nsites=ns, tol=TOL, itmax=ITMAX)
        b = ctx.batch_cond(L.SITE, it, site_orders=ref["so"], item_nsites=ns, tol=TOL, itmax=ITMAX)
    assert a == b  # two runs: bitwise
    assert a[0] == a[299] and a[0]["status"] == 0 and a[0]["iter"] > 0


def test_fast_order_accuracy():
    """the fast order against the literal result at the same tol, by the
    project's bar (test_batch.check_accuracy: 2 trunc + max(1e-10, tol), trunc
    from a literal run at tol 1e-13)"""
    lat = (0, 50, 50, 0)
    ref = reference(lat, L.SITE)
    cur = L.CUR_MATLAB
    with api.Context(*lat) as ctx:
        out = run(ctx, L.SITE, ref, tol=TOL, itmax=ITMAX)
        ctx.set_dot_order(L.DOT_LITERAL)
        tight = run(ctx, L.SITE, ref, tol=TIGHT, itmax=TIGHT_ITMAX)
    worst, solved = 0.0, 0
    for i, (o, c) in enumerate(zip(out, ref["cond"])):
        assert o["status"] == c[cur]["status"]
        d = TB.check_accuracy(o, c[cur], tight[i], (int(ref["trial"][i]), int(ref["ns"][i])))
        solved += c[cur]["status"] == 0
        worst = max(worst, d)
    print("worst relative distance to the literal result: %.3e over %d solved items" % (worst, solved))
    assert solved >= 25


def edge_items(kind, t, nb):
    if kind == L.SITE:
        return [(int(0.66 * t), 0), (t, 0)]
    return [(int(0.9 * t), int(0.8 * nb)), (t, nb)]


@pytest.mark.parametrize("kind", KINDS, ids=KIND_NAME.get)
@pytest.mark.parametrize("m,n", [(64, 130), (90, 93)])
def test_size_edges_literal_bitwise(m, n, kind):
    """N = 8192 (the cap, 1024 threads) and N = 8190 (a ragged last thread
    row): site at ps = 0.66 and 1.0, mixed at (0.9, 0.8) and (1.0, 1.0)"""
    with api.Context(0, m, n, 0) as ctx:
        t, nb = ctx.t, ctx.nb
        so = api.shuffled_ids(t, int(api.trial_seeds(58302 if kind == L.SITE else 143285, 1)[0]))
        bo = api.shuffled_ids(nb, int(api.trial_seeds(43716, 1)[0])) if kind == L.SITEBOND else None
        ctx.set_dot_order(L.DOT_LITERAL)
        items = edge_items(kind, t, nb)
        cur = L.CUR_MATLAB
        out = ctx.batch_cond(kind, [0, 0], site_orders=so, bond_orders=bo, item_nsites=[x[0] for x in items],
                             item_nbonds=[x[1] for x in items] if bo is not None else None, tol=TOL,
                             itmax=ITMAX)
        for o, (ns, nbc) in zip(out, items):
            li, c = single(ctx, kind, so, ns, bo, nbc)
            assert li["nspan"] == 1
            for k in LABEL_KEYS:
                assert o[k] == li[k], (k, ns, nbc, o, li)
            for k in COND_KEYS:
                assert o[k] == c[cur][k], (k, ns, nbc, o, c[cur])


def test_largest_labeling_view_literal_bitwise():
    """triangular 64 x 130 pbc: the largest bocc and socc labeling view"""
    with api.Context(1, 64, 130, 1) as ctx:
        t = ctx.t
        so = api.shuffled_ids(t, int(api.trial_seeds(58302, 1)[0]))
        ctx.set_dot_order(L.DOT_LITERAL)
        ns = int(0.66 * t)
        o = ctx.batch_cond(L.SITE, [0], site_orders=so, item_nsites=[ns], tol=TOL, itmax=ITMAX)[0]
        li, c = single(ctx, L.SITE, so, ns)
        for k in LABEL_KEYS:
            assert o[k] == li[k], (k, o, li)
        if li["nspan"] > 1:
            assert o["fallback"] == 1
        for k in COND_KEYS:
            assert o[k] == c[L.CUR_MATLAB][k], (k, o, c[L.CUR_MATLAB])


def column_sites(m, n, col):
    return [r * m + col + 1 for r in range(n)]


def test_spill_slot():
    """the shuffle's spill entry 0 inside the occupied prefix takes a
    position and is no site"""
    m = n = 8
    t = m * n
    col = column_sites(m, n, 3)
    ids = col[:2] + [0] + col[2:] + [k for k in range(1, t + 1) if k not in col]
    order = np.array(ids, np.int32)
    assert len(order) == t + 1 and order[2] == 0
    counts = [2, 3, 4, 8, 9, t, t + 1]
    with api.Context(0, m, n, 0) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        out = ctx.batch_cond(L.SITE, [0] * len(counts), site_orders=order, item_nsites=counts, tol=TOL,
                             itmax=ITMAX)
        spans = []
        for o, c in zip(out, counts):
            li, cr = single(ctx, L.SITE, order, c)
            for k in LABEL_KEYS:
                assert o[k] == li[k], (k, c, o, li)
            for k in COND_KEYS:
                assert o[k] == cr[L.CUR_MATLAB][k], (k, c, o, cr)
            spans.append(li["nspan"])
            assert (o["nspan"] > 0) == (li["nspan"] > 0)
    # 8 entries hold 7 sites of the column, 9 hold all 8 (the single path's count)
    assert spans[3] == 0 and spans[4] == 1 and spans[0] == 0 and spans[-1] == spans[-2] == 1


def test_forced_fallback():
    """two columns span at once: the reference's lowest-label rule through
    the single path"""
    m = n = 8
    t = m * n
    c0, c7 = column_sites(m, n, 0), column_sites(m, n, 7)
    rest = [k for k in range(1, t + 1) if k not in c0 and k not in c7]
    order = np.array(c0 + c7 + rest + [0], np.int32)
    cur = L.CUR_MATLAB
    with api.Context(0, m, n, 0) as ctx:
        for solve in (False, True):
            o = ctx.batch_cond(L.SITE, [0], site_orders=order, item_nsites=[16], solve=solve, tol=TOL,
                               itmax=ITMAX)[0]
            li, cr = single(ctx, L.SITE, order, 16, solve=solve)
            assert o["nspan"] == li["nspan"] == 2 and o["fallback"] == 1
            for k in LABEL_KEYS:
                assert o[k] == li[k], (k, o, li)
            if solve:
                for k in COND_KEYS:
                    assert o[k] == cr[cur][k], (k, o, cr[cur])
                assert o["gtop"] > 0.0
        # the other spanning column first: span_root changes exactly as the single path's
        order2 = np.array(c7 + c0 + rest + [0], np.int32)
        o2 = ctx.batch_cond(L.SITE, [0], site_orders=order2, item_nsites=[16], solve=False)[0]
        li2, _ = single(ctx, L.SITE, order2, 16, solve=False)
        assert o2["fallback"] == 1 and o2["span_root"] == li2["span_root"]
        assert (o2["span_root"] != o["span_root"]) == (li2["span_root"] != li["span_root"])
        # mixed kind: both columns' sites and every bond
        bo = api.shuffled_ids(ctx.nb, 7)
        om = ctx.batch_cond(L.SITEBOND, [0], site_orders=order, bond_orders=bo, item_nsites=[16],
                            item_nbonds=[ctx.nb + 1], tol=TOL, itmax=ITMAX)[0]
        lim, cm = single(ctx, L.SITEBOND, order, 16, bo, ctx.nb + 1)
        assert om["nspan"] == lim["nspan"] == 2 and om["fallback"] == 1
        for k in LABEL_KEYS:
            assert om[k] == lim[k], (k, om, lim)
        for k in COND_KEYS:
            assert om[k] == cm[cur][k], (k, om, cm[cur])


def test_errors_are_einval():
    with api.Context(0, 91, 93, 0) as ctx:
        so = api.shuffled_ids(ctx.t, 1)
        with pytest.raises(L.PercError, match="PERC_EINVAL"):
            ctx.batch_cond(L.SITE, [0], site_orders=so, item_nsites=[ctx.t // 2])
    with api.Context(0, 10, 10, 0) as ctx:
        t, nb = ctx.t, ctx.nb
        so, bo = api.shuffled_ids(t, 1), api.shuffled_ids(nb, 2)
        site = dict(site_orders=so, item_nsites=[5])
        mixed = dict(site_orders=so, bond_orders=bo, item_nsites=[5], item_nbonds=[5])
        ok = ctx.batch_cond(L.SITE, [0], **site)
        assert len(ok) == 1
        bad = [
            (L.SITE, [0], dict(site, rule=L.RULE_BOND)),          # a (kind, rule) pair outside the table
            (L.SITE, [0], dict(site, rule=L.RULE_MIXED)),
            (L.SITEBOND, [0], dict(mixed, rule=L.RULE_SITE)),
            (L.BOND, [0], dict(bond_orders=bo, item_nbonds=[5], rule=L.RULE_SITE)),
            (L.BONDSITE, [0], dict(mixed, rule=L.RULE_MIXED)),
            (L.SITE, [0], dict(site, cur_rule=2)),                # cur_rule
            (L.SITE, [0], dict(site, cur_rule=-1)),
            (L.SITE, [0], dict(site, itol=3)),                    # itol
            (L.SITE, [0], dict(site, itol=4)),
            (L.SITE, [0], dict(item_nsites=[5])),                 # a missing order list
            (L.SITEBOND, [0], dict(site_orders=so, item_nsites=[5], item_nbonds=[5])),
            (L.SITEBOND, [0], dict(bond_orders=bo, item_nsites=[5], item_nbonds=[5])),
            (L.BOND, [0], dict(item_nbonds=[5])),
            (L.SITE, [0], dict(site_orders=so)),                  # a missing count list
            (L.SITEBOND, [0], dict(site_orders=so, bond_orders=bo, item_nsites=[5])),
            (L.SITEBOND, [0], dict(site_orders=so, bond_orders=bo, item_nbonds=[5])),
            (L.BOND, [0], dict(bond_orders=bo)),
            (L.SITE, [1], site),                                  # a trial out of range
            (L.SITE, [-1], site),
            (L.SITE, [0], dict(site_orders=so, item_nsites=[t + 2])),  # a count out of range
            (L.SITE, [0], dict(site_orders=so, item_nsites=[-1])),
            (L.SITEBOND, [0], dict(mixed, item_nbonds=[nb + 2])),
            (L.SITEBOND, [0], dict(mixed, item_nbonds=[-1])),
            (L.SITEBOND, [0], dict(mixed, item_nsites=[t + 2])),
            (L.BOND, [0], dict(bond_orders=bo, item_nbonds=[nb + 2])),
        ]
        for kind, tr, kw in bad:
            with pytest.raises(L.PercError, match="PERC_EINVAL"):
                ctx.batch_cond(kind, tr, **kw)
            assert L.lib().perc_last_error().decode().startswith("perc_batch_cond:"), (kind, tr, kw)
        # ntrials or nitems below 0 (the C entry itself); an empty call is PERC_OK
        lib = L.lib()
        one = np.zeros(1, np.int32)
        out = (L.BatchItem * 1)()

        def call(ntrials, nitems):
            return lib.perc_batch_cond(ctx.h, L.SITE, L.RULE_SITE, L.CUR_MATLAB, ntrials, L.ptr(so), None, nitems,
                                       L.ptr(one), L.ptr(one), None, 1, 1.0, 1.0, api.LEAK, 2, TOL, ITMAX,
                                       C.cast(out, C.c_void_p))

        assert call(-1, 0) == -1 and call(1, -1) == -1
        assert call(1, 0) == L.PERC_OK and call(0, 0) == L.PERC_OK
        assert ctx.batch_cond(L.SITE, [], site_orders=so, item_nsites=[]) == []


def test_cond_curve_batched_equals_unbatched():
    lat = (0, 10, 10, 0)
    cases = [(L.SITE, [0.5, 0.6, 0.7, 0.8, 0.9, 1.0], 58302),
             (L.SITEBOND, [(ps, pb) for ps in (0.8, 1.0) for pb in (0.5, 0.7, 0.9)], 8811064)]
    for kind, grid, master in cases:
        res = {}
        for batch in (64, 0):
            with api.Context(*lat) as ctx:
                ctx.set_dot_order(L.DOT_LITERAL)
                res[batch] = api.cond_curve(*lat, kind=kind, grid=grid, master=master, numtrials=3,
                                            batch=batch, ctx=ctx)
        (ra, sa), (rb, sb) = res[64], res[0]
        assert ra == rb and len(ra) == 3 and all(len(tr["rows"]) == len(grid) for tr in ra)
        assert sa.shape == sb.shape == (len(grid), 5)
        assert sa.tobytes() == sb.tobytes()
        assert (sa[:, 0] == 3).all()
        assert sa[:, 3].any() and not (sa[:, 3] == 3).all()  # spanning counts: not all zero, not all numtrials
        # the rows are batch_cond's items of the same orders
        seeds = api.trial_seeds(master, 3) if kind == L.SITE else None
        if seeds is not None:
            assert [tr["seed"] for tr in ra] == [int(s) for s in seeds]
            assert [r["nsites"] for r in ra[0]["rows"]] == [int(p * 100) for p in grid]
