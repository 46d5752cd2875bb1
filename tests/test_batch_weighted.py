"""The batch path with per-bond conductance multipliers
(perc_batch_cond_weighted: k_twister_stream, k_batch_cond_w), ConductCalc.m
condtype 2 for ensembles of small lattices:

* the device generator against perc_twister_uniform, bit for bit;
* explicit weight rows and ConductCalc seeds in the literal dot order against
  the single path (perc_set_bond_weights / perc_set_conductcalc_weights +
  perc_conductance), item by item, all three kinds, both current rules, on
  10 x 10 / 12 x 10 grids and a handful of 50 x 50 items;
* a row of 1.0 against the unweighted perc_batch_cond, bitwise;
* the oracle's linbcg and currents on gval = -g0 w;
* weights that put bonds below the Fortran rule's 1e-10 threshold;
* the fast order (deterministic, position independent, accurate), a call cut
  into two launches, the forced fallback, every PERC_EINVAL case and
  api.cond_curve(condtype=2).

The single-path reference of a (lattice, kind) is computed once and shared."""
import ctypes as C

import numpy as np
import pytest

import rule_systems as R
import test_batch as TB
import test_batch_cond as TBC
from percolation_amd import _lib as L
from percolation_amd import api

pytestmark = pytest.mark.gpu
TOL, ITMAX = 1e-8, 2500
TIGHT, TIGHT_ITMAX = 1e-13, 20000
SMALL = [(0, 10, 10, 0), (0, 10, 10, 1), (1, 10, 10, 0), (1, 12, 10, 1)]
BIG = [(0, 50, 50, 0), (1, 50, 50, 0)]
LATTICES = SMALL + BIG
KINDS = [L.BOND, L.SITE, L.SITEBOND]
KIND_NAME = {L.BOND: "bond", L.SITE: "site", L.SITEBOND: "mixed"}
CURS = [L.CUR_FORTRAN, L.CUR_MATLAB]
LABEL_KEYS = TBC.LABEL_KEYS
COND_KEYS = TBC.COND_KEYS
SEED0 = 7000


def items_of(kind, lat):
    """the orders and the items (trial, nsites, nbonds) of a lattice:
    test_batch_cond.items_of's grids (bond: test_batch.reference's, every
    pb_grid count of three trials); on 50 x 50 six items of trial 0"""
    t, nb = lat[1] * lat[2], api.nbonds(*lat)
    if kind == L.BOND:
        ss, bs = None, api.trial_seeds(58302, 3)
        counts = sorted({int(c) for c in api.pb_grid(lat[0], nb) if 0 < c <= nb} | {0, 1, nb, nb + 1})
        items = [(tr, 0, c) for tr in range(3) for c in counts]
    else:
        (ss, bs), items = TBC.items_of(kind, lat)
    if lat in BIG:
        first = [x for x in items if x[0] == 0]
        if kind == L.BOND:
            pick = [min(first, key=lambda x: abs(x[2] - p * nb)) for p in (0.45, 0.55, 0.6, 0.7, 0.85, 1.0)]
        elif kind == L.SITE:
            pick = [min(first, key=lambda x: abs(x[1] - p * t)) for p in (0.55, 0.65, 0.7, 0.8, 0.9, 1.0)]
        else:
            pick = [x for x in first if x[1] >= round(0.9 * t) and x[2] >= round(0.8 * nb)]
        items = pick
    so = np.stack([api.shuffled_ids(t, int(s)) for s in ss]) if ss is not None else None
    bo = np.stack([api.shuffled_ids(nb, int(s)) for s in bs]) if bs is not None else None
    return so, bo, items


def occupy(ctx, kind, so, bo, item):
    tr, ns, nbc = item
    if kind == L.BOND:
        o, k = TBC.prefix(bo[tr], nbc, ctx.nb)
        ctx.occupy(L.BOND, bond_order=o, nbonds_=k)
    else:
        TBC.occupy(ctx, kind, so[tr], ns, None if bo is None else bo[tr], nbc)


def solve_both(ctx, kind, Va=1.0, g0=1.0, leak=api.LEAK, tol=TOL, itmax=ITMAX):
    """perc_conductance on the context as it stands, per current rule (one
    solve; the other rule's currents of the same voltages by perc_currents)"""
    rule = api.KIND_RULE[kind]
    c = ctx.conductance(rule, L.CUR_MATLAB, Va, g0, leak, 2, tol, itmax)
    f = dict(c)
    if c["status"] == 0:
        res = L.CondResult()
        L.check(L.lib().perc_currents(ctx.h, rule, L.CUR_FORTRAN, Va, g0, leak, C.byref(res)), "perc_currents")
        f["gtop"], f["gbot"] = res.gtop, res.gbot
    return {L.CUR_MATLAB: c, L.CUR_FORTRAN: f}


_REF = {}


def reference(lat, kind):
    """orders, items, two weight rows (uniform over every bond; item i uses
    row i % 2), one seed per item (the second item one cluster spans shares
    the first one's) and the single path's labels and literal conductances
    under the explicit row and under the seed, computed once"""
    if (lat, kind) in _REF:
        return _REF[lat, kind]
    so, bo, items = items_of(kind, lat)
    rule = api.KIND_RULE[kind]
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        W = np.random.RandomState(20240 + 7 * kind + lat[1]).random_sample((2, ctx.nb))
        lab, expl, cc, seeds, shared = [], [], [], [], None
        for i, item in enumerate(items):
            occupy(ctx, kind, so, bo, item)
            li = ctx.label()
            seed = SEED0 + i
            if li["nspan"] == 1 and shared is None:
                shared = seed
            elif li["nspan"] == 1 and shared >= 0:
                seed, shared = shared, -1
            ctx.set_bond_weights(W[i % 2])
            expl.append(solve_both(ctx, kind))
            ctx.set_conductcalc_weights(rule, seed)
            cc.append(solve_both(ctx, kind))
            ctx.set_bond_weights(None)
            lab.append(li)
            seeds.append(seed)
    _REF[lat, kind] = dict(
        so=so, bo=bo, trial=np.array([x[0] for x in items], np.int32),
        ns=np.array([x[1] for x in items], np.int32) if kind != L.BOND else None,
        nb=np.array([x[2] for x in items], np.int32) if kind != L.SITE else None,
        W=W, wset=np.arange(len(items), dtype=np.int32) % 2, seeds=np.array(seeds, np.int64),
        label=lab, expl=expl, cc=cc)
    return _REF[lat, kind]


def run(ctx, kind, ref, **kw):
    return ctx.batch_cond(kind, ref["trial"], site_orders=ref["so"], bond_orders=ref["bo"],
                          item_nsites=ref["ns"], item_nbonds=ref["nb"], **kw)


def check_against_single(lat, kind, cur, ref, out, want, plain):
    """out item by item the single path's weighted records; the bar on the
    items one cluster spans (the ones that exercise the kernel)"""
    assert len(out) == len(ref["label"]) == len(plain)
    once = 0
    for i, (o, li, c) in enumerate(zip(out, ref["label"], want)):
        what = (i, int(ref["trial"][i]), o, c[cur])
        for k in LABEL_KEYS:
            assert o[k] == li[k], (k,) + what
        for k in COND_KEYS:
            assert o[k] == c[cur][k], (k,) + what
        if li["nspan"] == 1:
            once += 1
            assert o["fallback"] == 0 and o["status"] == 0 and o["iter"] > 0, what
            assert o["gtop"] != plain[i]["gtop"], what
    print("lattice %s %s: %d of %d items span once" % (lat, KIND_NAME[kind], once, len(out)))
    assert once >= (3 if lat in BIG else 10)


# ---------------------------------------------------------------- 1. the generator
def test_twister_stream_bitwise():
    seeds = [0, 1, 1838534, 0xFFFFFFFF]
    with api.Context(0, 10, 10, 0) as ctx:
        for n in (1, 311, 312, 313, 624, 5000):
            got = ctx.batch_twister(seeds, n)
            assert got.shape == (4, n)
            for k, s in enumerate(seeds):
                assert got[k].tobytes() == api.twister_uniform(s, n).tobytes(), (s, n)
        two = ctx.batch_twister([1838534, 5, 1838534], 700)
        assert two[0].tobytes() == two[2].tobytes() and two[0].tobytes() != two[1].tobytes()
        assert ctx.batch_twister([], 5).shape == (0, 5) and ctx.batch_twister([3], 0).shape == (1, 0)
    assert np.array_equal(got[2], np.random.RandomState(1838534).random_sample(5000))


# ---------------------------------------------------------------- 2. explicit rows
@pytest.mark.parametrize("cur", CURS, ids=["fortran", "matlab"])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_NAME.get)
@pytest.mark.parametrize("lat", LATTICES)
def test_explicit_weights_literal_bitwise(lat, kind, cur):
    ref = reference(lat, kind)
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        out = run(ctx, kind, ref, cur_rule=cur, tol=TOL, itmax=ITMAX, weights=ref["W"], item_wset=ref["wset"])
        plain = run(ctx, kind, ref, cur_rule=cur, tol=TOL, itmax=ITMAX)
    check_against_single(lat, kind, cur, ref, out, ref["expl"], plain)


# ---------------------------------------------------------------- 3. a row of 1.0
@pytest.mark.parametrize("kind", KINDS, ids=KIND_NAME.get)
@pytest.mark.parametrize("lat", [(0, 10, 10, 1), (1, 12, 10, 1), (1, 50, 50, 0)])
def test_unit_weights_are_the_unweighted_batch(lat, kind):
    """-g0 * 1.0 == -g0 and the sums run in the same order"""
    ref = reference(lat, kind)
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        for cur in CURS:
            got = run(ctx, kind, ref, cur_rule=cur, tol=TOL, itmax=ITMAX, weights=np.ones(ctx.nb),
                      item_wset=np.zeros(len(ref["trial"]), np.int32))
            want = run(ctx, kind, ref, cur_rule=cur, tol=TOL, itmax=ITMAX)
            assert got == want
            assert sum(w["status"] == 0 and w["iter"] > 0 and w["fallback"] == 0 for w in want) >= 3


# ---------------------------------------------------------------- 4. ConductCalc seeds
@pytest.mark.parametrize("cur", CURS, ids=["fortran", "matlab"])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_NAME.get)
@pytest.mark.parametrize("lat", LATTICES)
def test_conductcalc_seeds_literal_bitwise(lat, kind, cur):
    ref = reference(lat, kind)
    seeds = ref["seeds"]
    once = [i for i, li in enumerate(ref["label"]) if li["nspan"] == 1]
    # one seed shared by two items of different occupancy, the others their own
    assert seeds[once[0]] == seeds[once[1]] and len(set(seeds.tolist())) == len(seeds) - 1
    a, b = once[0], once[1]
    key = [(int(ref["trial"][i]), None if ref["ns"] is None else int(ref["ns"][i]),
            None if ref["nb"] is None else int(ref["nb"][i])) for i in (a, b)]
    assert key[0] != key[1]
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        out = run(ctx, kind, ref, cur_rule=cur, tol=TOL, itmax=ITMAX, item_wseed=seeds)
        plain = run(ctx, kind, ref, cur_rule=cur, tol=TOL, itmax=ITMAX)
    check_against_single(lat, kind, cur, ref, out, ref["cc"], plain)


# ---------------------------------------------------------------- 5. the oracle
ORACLE_SYSTEMS = [R.System(rule, *g, *v) for rule in sorted(R.RULE_NAME) for g in (R.G_SMALL_SQ, R.G_SMALL_TRI)
                  for v in (R.UNIT, R.LEAK_DROPPED)]
RULE_KIND = {L.RULE_BOND: L.BOND, L.RULE_SITE: L.SITE, L.RULE_MIXED: L.SITEBOND}


@pytest.mark.parametrize("s", ORACLE_SYSTEMS, ids=R.name)
def test_oracle_linbcg_and_currents_bitwise(s):
    """one item per system in the literal order: iter and err the oracle's
    linbcg's on gval = -g0 w, Gtop and Gbot its currents under both rules --
    the weights as an explicit row and drawn from the seed on the device"""
    seed = 1838534
    d = R.build(s)
    assert d["nspan"] == 1
    occ = d["occ"]
    kind = RULE_KIND[s.rule]
    assert occ["kind"] == kind
    w = api.conductcalc_weights(s.rule, d["b1"], d["b2"], d["blabel"],
                                d["slabel"] if s.rule != L.RULE_BOND else None, d["perccln"], seed)
    gval = d["gval"].copy()
    inc = gval == -s.g0
    assert inc.sum() > 100 and (w[~inc] == 1.0).all() and (w[inc] < 1.0).all()
    gval[inc] = -s.g0 * w[inc]
    oc = R.oracle_conductance(s, d, TOL, gval)
    assert oc["iter"] < R.ITMAX and oc["err"] <= TOL
    with api.Context(*R.geometry(s)) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        for cur in CURS:
            for mode in (dict(weights=w, item_wset=[0]), dict(item_wseed=[seed])):
                o = ctx.batch_cond(kind, [0], site_orders=occ.get("site_order"), bond_orders=occ.get("bond_order"),
                                   item_nsites=[occ["nsites"]] if kind != L.BOND else None,
                                   item_nbonds=[occ["nbonds_"]] if kind != L.SITE else None, rule=s.rule,
                                   cur_rule=cur, Va=s.Va, g0=s.g0, leak=s.leak, tol=TOL, itmax=R.ITMAX, **mode)[0]
                what = (cur, sorted(mode), o, oc["iter"], oc["err"], oc["cur"][cur])
                assert o["nspan"] == 1 and o["fallback"] == 0 and o["status"] == 0, what
                assert o["iter"] == oc["iter"] and o["err"] == oc["err"], what
                assert (o["gtop"], o["gbot"]) == oc["cur"][cur], what


# ---------------------------------------------------------------- 6. small weights
@pytest.mark.parametrize("lat", [(0, 10, 10, 0), (1, 12, 10, 1)])
def test_weights_below_the_current_threshold(lat):
    """a few in-cluster bonds at 1e-11 / g0, one of them on an electrode row:
    the Fortran rule's |G| >= 1e-10 test drops their terms"""
    g0, Va, leak = 2.5, 0.7, 3e-11
    with api.Context(*lat) as ctx:
        t, nb, m = ctx.t, ctx.nb, ctx.m
        b1, b2 = api.bond_list(*lat)
        so = api.shuffled_ids(t, 11)
        w = np.random.RandomState(3).random_sample(nb)
        bottom = [k for k in range(nb) if b1[k] <= m and b2[k] > m]
        top = [k for k in range(nb) if b2[k] > t - m and b1[k] <= t - m]
        inner = [k for k in range(nb) if 2 * m < b1[k] and b2[k] <= t - 2 * m]
        small = [bottom[3], top[1], inner[0], inner[len(inner) // 2], inner[-1]]
        w[small] = 1e-11 / g0
        assert (g0 * w[small] < 1e-10).all()
        ctx.set_dot_order(L.DOT_LITERAL)
        got = {cur: ctx.batch_cond(L.SITE, [0], site_orders=so, item_nsites=[t], cur_rule=cur, Va=Va, g0=g0,
                                   leak=leak, tol=TOL, itmax=ITMAX, weights=w, item_wset=[0])[0] for cur in CURS}
        TBC.occupy(ctx, L.SITE, so, t)
        li = ctx.label()
        assert li["nspan"] == 1 and li["span_sites"] == t  # every bond is the cluster's
        ctx.set_bond_weights(w)
        want = solve_both(ctx, L.SITE, Va, g0, leak)
        ctx.set_bond_weights(None)
    for cur in CURS:
        assert got[cur]["status"] == 0 and got[cur]["iter"] > 0 and got[cur]["fallback"] == 0
        for k in COND_KEYS:
            assert got[cur][k] == want[cur][k], (cur, k, got[cur], want[cur])
    assert got[L.CUR_FORTRAN]["iter"] == got[L.CUR_MATLAB]["iter"]  # one solve, two current rules


# ---------------------------------------------------------------- 7. the fast order
def fast_items():
    """300 site items on 50 x 50, the same item (and seed) first and last"""
    lat = (0, 50, 50, 0)
    t = 2500
    (ss, _), items = TBC.items_of(L.SITE, lat)
    so = np.stack([api.shuffled_ids(t, int(s)) for s in ss])
    grid = sorted({x[1] for x in items if 0 < x[1] <= t})
    probe = (0, int(round(0.70 * t)))
    its = [probe] + [(i % 3, grid[(7 * i) % len(grid)]) for i in range(1, 299)] + [probe]
    seeds = [SEED0] + [SEED0 + i for i in range(1, 299)] + [SEED0]
    return lat, so, np.array([x[0] for x in its], np.int32), np.array([x[1] for x in its], np.int32), seeds


def test_fast_order_deterministic_and_position_independent():
    lat, so, it, ns, seeds = fast_items()
    assert len(it) == 300
    with api.Context(*lat) as ctx:
        a = ctx.batch_cond(L.SITE, it, site_orders=so, item_nsites=ns, tol=TOL, itmax=ITMAX, item_wseed=seeds)
        b = ctx.batch_cond(L.SITE, it, site_orders=so, item_nsites=ns, tol=TOL, itmax=ITMAX, item_wseed=seeds)
    assert a == b  # two runs: bitwise
    assert a[0] == a[299] and a[0]["status"] == 0 and a[0]["iter"] > 0 and a[0]["fallback"] == 0


@pytest.mark.parametrize("mode", ["explicit", "seeds"])
def test_fast_order_accuracy(mode):
    """the fast order against the literal result at the same tol, by the
    project's bar (test_batch.check_accuracy: 2 trunc + max(1e-10, tol), trunc
    from a literal run at tol 1e-13)"""
    lat, so, it, ns, seeds = fast_items()
    it, ns, seeds = it[:75], ns[:75], seeds[:75]
    if mode == "explicit":
        W = np.random.RandomState(5).random_sample((2, api.nbonds(*lat)))
        kw = dict(weights=W, item_wset=np.arange(75, dtype=np.int32) % 2)
    else:
        kw = dict(item_wseed=seeds)
    with api.Context(*lat) as ctx:
        fast = ctx.batch_cond(L.SITE, it, site_orders=so, item_nsites=ns, tol=TOL, itmax=ITMAX, **kw)
        ctx.set_dot_order(L.DOT_LITERAL)
        lit = ctx.batch_cond(L.SITE, it, site_orders=so, item_nsites=ns, tol=TOL, itmax=ITMAX, **kw)
        tight = ctx.batch_cond(L.SITE, it, site_orders=so, item_nsites=ns, tol=TIGHT, itmax=TIGHT_ITMAX, **kw)
    worst, solved = 0.0, 0
    for i, (o, c) in enumerate(zip(fast, lit)):
        assert o["status"] == c["status"] and o["nspan"] == c["nspan"]
        if c["status"] == 0 and c["iter"] > 0:
            worst = max(worst, TB.check_accuracy(o, c, tight[i], (i, int(it[i]), int(ns[i]))))
            solved += 1
    print("worst relative distance to the literal result: %.3e over %d solved items" % (worst, solved))
    assert solved >= 25


@pytest.mark.parametrize("mode", ["explicit", "seeds"])
def test_second_launch_of_a_call_reads_its_own_weights(mode):
    """more items than one launch takes (16384): the items past the cut get
    their own rows / seeds, not the first launch's"""
    lat = (0, 10, 10, 0)
    n = 16384 + 6
    so = np.stack([api.shuffled_ids(100, int(s)) for s in api.trial_seeds(58302, 3)])
    it = (np.arange(n) % 3).astype(np.int32)
    ns = np.full(n, 100, np.int32)  # every site: one cluster, no fallback
    with api.Context(*lat) as ctx:
        if mode == "explicit":
            W = np.random.RandomState(8).random_sample((7, ctx.nb))
            sel = (np.arange(n) % 7).astype(np.int32)
            kw = lambda s: dict(weights=W, item_wset=sel[s])
        else:
            seeds = SEED0 + np.arange(n, dtype=np.int64) % 1000
            kw = lambda s: dict(item_wseed=seeds[s])
        whole = slice(0, n)
        tail = slice(16384 - 3, n)
        a = ctx.batch_cond(L.SITE, it, site_orders=so, item_nsites=ns, tol=TOL, itmax=ITMAX, **kw(whole))
        b = ctx.batch_cond(L.SITE, it[tail], site_orders=so, item_nsites=ns[tail], tol=TOL, itmax=ITMAX, **kw(tail))
    assert a[tail] == b and len(b) == 9
    assert sum(o["status"] == 0 and o["iter"] > 0 and o["fallback"] == 0 for o in b) >= 6
    assert len({o["gtop"] for o in b}) >= 6  # different weights, different conductances


# ---------------------------------------------------------------- 8. the fallback
@pytest.mark.parametrize("mode", ["explicit", "seeds"])
def test_forced_fallback(mode):
    """two columns span at once: the single path's weighted record, and the
    context unweighted afterwards"""
    m = n = 8
    t = m * n
    c0, c7 = TBC.column_sites(m, n, 0), TBC.column_sites(m, n, 7)
    rest = [k for k in range(1, t + 1) if k not in c0 and k not in c7]
    order = np.array(c0 + c7 + rest + [0], np.int32)
    cur = L.CUR_MATLAB
    seed = 4242
    with api.Context(0, m, n, 0) as ctx, api.Context(0, m, n, 0) as other:
        w = np.random.RandomState(9).random_sample(ctx.nb)
        kw = dict(weights=w, item_wset=[0]) if mode == "explicit" else dict(item_wseed=[seed])
        for c in (ctx, other):
            c.set_dot_order(L.DOT_LITERAL)
        o = ctx.batch_cond(L.SITE, [0], site_orders=order, item_nsites=[16], tol=TOL, itmax=ITMAX, **kw)[0]
        after = ctx.conductance(L.RULE_SITE, cur, 1.0, 1.0, api.LEAK, 2, TOL, ITMAX)  # the item's labeling, no weights
        TBC.occupy(other, L.SITE, order, 16)
        li = other.label()
        plain = other.conductance(L.RULE_SITE, cur, 1.0, 1.0, api.LEAK, 2, TOL, ITMAX)
        if mode == "explicit":
            other.set_bond_weights(w)
        else:
            other.set_conductcalc_weights(L.RULE_SITE, seed)
        want = other.conductance(L.RULE_SITE, cur, 1.0, 1.0, api.LEAK, 2, TOL, ITMAX)
        # solve = 0: the labels only, no weights touched
        o0 = ctx.batch_cond(L.SITE, [0], site_orders=order, item_nsites=[16], solve=False, **kw)[0]
    assert o["nspan"] == li["nspan"] == 2 and o["fallback"] == 1 and o0["fallback"] == 1
    for k in LABEL_KEYS:
        assert o[k] == li[k] == o0[k], (k, o, li, o0)
    for k in COND_KEYS:
        assert o[k] == want[k], (k, o, want)
        assert after[k] == plain[k], (k, after, plain)
    assert o["gtop"] != plain["gtop"] and o["gtop"] > 0.0


# ---------------------------------------------------------------- 9. arguments
def test_errors_are_einval():
    lib = L.lib()
    with api.Context(0, 128, 128, 0) as ctx:  # the large kernel's lattice, not this one's
        so = api.shuffled_ids(ctx.t, 1)
        with pytest.raises(L.PercError, match="PERC_EINVAL"):
            ctx.batch_cond(L.SITE, [0], site_orders=so, item_nsites=[ctx.t // 2], item_wseed=[1])
        assert "perc_batch_weighted_supported" in lib.perc_last_error().decode()
        ctx.set_batch_large(True)
        with pytest.raises(L.PercError, match="PERC_EINVAL"):
            ctx.batch_cond(L.SITE, [0], site_orders=so, item_nsites=[ctx.t // 2], item_wseed=[1])
        assert "perc_batch_weighted_supported" in lib.perc_last_error().decode()
    with api.Context(0, 10, 10, 0) as ctx:
        t, nb = ctx.t, ctx.nb
        so, bo = api.shuffled_ids(t, 1), api.shuffled_ids(nb, 2)
        w = np.ones((2, nb))
        site = dict(site_orders=so, item_nsites=[60])
        ok = ctx.batch_cond(L.SITE, [0], **site, weights=w, item_wset=[1])
        assert len(ok) == 1
        bad = [
            dict(site, weights=w, item_wset=[0], item_wseed=[1]),  # both inputs
            dict(site, weights=w),                                 # weights without item_wset
            dict(site, item_wset=[0]),                             # ... and the reverse
            dict(site, weights=w, item_wset=[2]),                  # a row out of range
            dict(site, weights=w, item_wset=[-1]),
            dict(site, item_wseed=[1], rule=L.RULE_BOND),          # perc_batch_cond's own cases
            dict(site, item_wseed=[1], cur_rule=2),
            dict(site, item_wseed=[1], itol=3),
            dict(item_nsites=[60], item_wseed=[1]),
            dict(site_orders=so, item_wseed=[1]),
            dict(site_orders=so, item_nsites=[t + 2], item_wseed=[1]),
        ]
        for kw in bad:
            with pytest.raises(L.PercError, match="PERC_EINVAL"):
                ctx.batch_cond(L.SITE, [0], **kw)
            assert lib.perc_last_error().decode().startswith("perc_batch_cond_weighted:"), kw
        with pytest.raises(L.PercError, match="PERC_EINVAL"):
            ctx.batch_cond(L.SITE, [1], **site, item_wseed=[1])
        one = np.zeros(1, np.int32)
        sixty = np.full(1, 60, np.int32)
        sd = np.ones(1, np.uint32)
        out = (L.BatchItem * 1)()

        def call(ntrials, nitems, nwsets, wp, ws, wd):
            return lib.perc_batch_cond_weighted(ctx.h, L.SITE, L.RULE_SITE, L.CUR_MATLAB, ntrials, L.ptr(so), None,
                                                nitems, L.ptr(one), L.ptr(sixty), None, nwsets, wp, ws, wd, 1,
                                                1.0, 1.0, api.LEAK, 2, TOL, ITMAX, C.cast(out, C.c_void_p))

        assert call(1, 1, 0, None, None, None) == -1          # neither input
        assert lib.perc_last_error().decode().startswith("perc_batch_cond_weighted:")
        assert call(1, 1, 0, L.ptr(w), L.ptr(one), None) == -1  # nwsets < 1 in explicit mode
        assert call(1, 1, -3, L.ptr(w), L.ptr(one), None) == -1
        assert call(-1, 0, 0, None, None, L.ptr(sd)) == -1 and call(1, -1, 0, None, None, L.ptr(sd)) == -1
        assert call(1, 1, 2, L.ptr(w), L.ptr(one), None) == L.PERC_OK
        assert call(1, 1, 0, None, None, L.ptr(sd)) == L.PERC_OK
        assert call(1, 0, 0, None, None, L.ptr(sd)) == L.PERC_OK and call(0, 0, 2, L.ptr(w), L.ptr(one), None) == L.PERC_OK
        assert ctx.batch_cond(L.SITE, [], site_orders=so, item_nsites=[], item_wseed=[]) == []
        with pytest.raises(ValueError):
            ctx.batch_cond(L.SITE, [0], site_seeds=[1], item_nsites=[60], item_wseed=[1])
        # the generator's own
        buf = np.zeros(4)
        assert lib.perc_batch_twister(ctx.h, -1, L.ptr(sd), 4, L.ptr(buf)) == -1
        assert lib.perc_last_error().decode().startswith("perc_batch_twister:")
        assert lib.perc_batch_twister(ctx.h, 1, L.ptr(sd), -1, L.ptr(buf)) == -1
        assert lib.perc_batch_twister(ctx.h, 0, None, 4, None) == L.PERC_OK
        assert lib.perc_batch_twister(ctx.h, 1, L.ptr(sd), 0, None) == L.PERC_OK


def test_batch_large_flag_is_not_read():
    lat, kind = (0, 10, 10, 1), L.SITEBOND
    ref = reference(lat, kind)
    with api.Context(*lat) as ctx:
        kw = dict(tol=TOL, itmax=ITMAX, item_wseed=ref["seeds"])
        a = run(ctx, kind, ref, **kw)
        ctx.set_batch_large(True)
        b = run(ctx, kind, ref, **kw)
        assert ctx.batch_large()
    assert a == b and sum(o["status"] == 0 and o["iter"] > 0 for o in a) >= 10


# ---------------------------------------------------------------- 10. cond_curve
def test_cond_curve_condtype2_batched_equals_unbatched():
    lat = (0, 10, 10, 0)
    cases = [(L.SITE, [0.6, 0.8, 1.0], 58302), (L.SITEBOND, [(0.9, 0.8), (1.0, 0.7), (1.0, 1.0)], 8811064)]
    for kind, grid, master in cases:
        res = {}
        for batch, condtype in ((64, 2), (0, 2), (64, 1)):
            with api.Context(*lat) as ctx:
                ctx.set_dot_order(L.DOT_LITERAL)
                res[batch, condtype] = api.cond_curve(*lat, kind=kind, grid=grid, master=master, numtrials=2,
                                                      batch=batch, ctx=ctx, condtype=condtype)
                # the context is left unweighted
                if condtype == 2:
                    again = api.cond_curve(*lat, kind=kind, grid=grid, master=master, numtrials=2, batch=0, ctx=ctx)
        (ra, sa), (rb, sb), (r1, s1) = res[64, 2], res[0, 2], res[64, 1]
        assert ra == rb and len(ra) == 2 and all(len(tr["rows"]) == 3 for tr in ra)
        assert sa.shape == (3, 5) and sa.tobytes() == sb.tobytes()
        assert again[0] == r1 and again[1].tobytes() == s1.tobytes()
        spanning = 0
        for ta, t1 in zip(ra, r1):
            for a, b in zip(ta["rows"], t1["rows"]):
                assert a["spanning"] == b["spanning"] and a["nsites"] == b["nsites"]
                if a["spanning"]:
                    spanning += 1
                    assert a["gtop"] != b["gtop"] and 0.0 < a["gtop"] < b["gtop"], (a, b)
                else:
                    assert a["gtop"] == b["gtop"] == 0.0
        assert spanning >= 3
        # another wseed: other draws
        with api.Context(*lat) as ctx:
            ctx.set_dot_order(L.DOT_LITERAL)
            rc, _ = api.cond_curve(*lat, kind=kind, grid=grid, master=master, numtrials=2, batch=64, ctx=ctx,
                                   condtype=2, wseed=99)
        assert rc != ra
