"""Batch current distributions (perc_batch_cond_currents, k_batch_cond's FIELDS
instantiations): the bond-current record and the interior voltages of every
item of a batch launch, against the single path (perc_occupy / perc_label /
perc_conductance(vint_out)) and the host's record (perc_current_stats_host,
itself checked against numpy in test_batch_currents_host):

* the literal dot order: `out` as perc_batch_cond fills it, the voltages
  bitwise the single path's, the record's counts, maximum and histogram those
  of the host's record on these voltages with the single path's conducting
  mask, its sums within (nbonds + 8) 2^-52 relative (bar 1: two orders of
  nbonds exactly equal terms, each within (nbonds - 1) 2^-53 of their exact
  sum) -- three kinds, both current rules, test_batch_cond's lattices and
  N = 8192 on 1024 threads;
* the fast order against the host's record on the call's own voltages;
  deterministic and independent of the item's place in the launch;
* records with and without the voltages, a voltage request that crosses a
  chunk boundary, the two-cluster fallback, an item nothing spans, the seeded
  call, non-unit Va / g0 / leak, cut = 0 and cut = 1, api.current_curve
  batched against unbatched, every PERC_EINVAL case.

The single-path reference of a (lattice, kind) is computed once and shared."""
import ctypes as C

import numpy as np
import pytest

import rule_systems as R
import test_batch_cond as TBC
import test_batch_currents_host as H
from percolation_amd import _lib as L
from percolation_amd import api

pytestmark = pytest.mark.gpu
TOL, ITMAX, CUT = TBC.TOL, TBC.ITMAX, 1e-6
KINDS = [L.BOND, L.SITE, L.SITEBOND]
KIND_NAME = {L.BOND: "bond", L.SITE: "site", L.SITEBOND: "mixed"}
CURS = TBC.CURS
ITEM_KEYS = tuple(k for k, _ in L.BatchItem._fields_)
INT_KEYS = ("nbonds", "nabove", "imax")
BIG = (0, 64, 130, 0)  # N = 8192: 1024 threads, 8 full rows each


def items(lat, kind):
    """dict(so, bo, trial, ns, nb): test_batch's three trials on a grid of
    counts for the bond kind, test_batch_cond's items (items_of) for the
    others; two items at pb = 0.60 on BIG"""
    if lat == BIG:
        nb = api.nbonds(*lat)
        bo = np.stack([api.shuffled_ids(nb, int(s)) for s in api.trial_seeds(58302, 2)])
        return dict(so=None, bo=bo, trial=np.array([0, 1], np.int32), ns=None,
                    nb=np.full(2, int(0.60 * nb), np.int32))
    if kind == L.BOND:  # pb = 0.35 .. 1.0, nothing, one bond, the whole order: 51 items
        nb = api.nbonds(*lat)
        bo = np.stack([api.shuffled_ids(nb, int(s)) for s in api.trial_seeds(58302, 3)])
        counts = sorted({int(round(0.05 * k * nb)) for k in range(7, 21)} | {0, 1, nb + 1})
        return dict(so=None, bo=bo, trial=np.repeat(np.arange(3, dtype=np.int32), len(counts)), ns=None,
                    nb=np.tile(np.array(counts, np.int32), 3))
    r = TBC.reference(lat, kind)
    return dict(so=r["so"], bo=r["bo"], trial=r["trial"], ns=r["ns"], nb=r["nb"])


def run(ctx, kind, it, sel=None, **kw):
    """batch_cond over the items (sel: a subset by index)"""
    pick = (lambda a: None if a is None else a[sel]) if sel is not None else (lambda a: a)
    return ctx.batch_cond(kind, pick(it["trial"]), site_orders=it["so"], bond_orders=it["bo"],
                          item_nsites=pick(it["ns"]), item_nbonds=pick(it["nb"]), tol=kw.pop("tol", TOL),
                          itmax=kw.pop("itmax", ITMAX), **kw)


def single_fields(ctx, kind, it, i, b1, b2, Va=1.0, g0=1.0, leak=api.LEAK, cur=L.CUR_MATLAB):
    """the single path on item i: (label, conductance with vint, conducting mask)"""
    tr = int(it["trial"][i])
    if kind == L.BOND:
        o, k = TBC.prefix(it["bo"][tr], int(it["nb"][i]), ctx.nb)
        ctx.occupy(L.BOND, bond_order=o, nbonds_=k)
    else:
        TBC.occupy(ctx, kind, it["so"][tr], int(it["ns"][i]), None if it["bo"] is None else it["bo"][tr],
                   0 if it["nb"] is None else int(it["nb"][i]))
    li = ctx.label(canon=True)
    c = ctx.conductance(api.KIND_RULE[kind], cur, Va, g0, leak, 2, TOL, ITMAX, vint=True)
    socc, bocc = ctx.occupancy()
    return li, c, api.conducting_bonds(kind, b1, b2, socc, bocc, li["canon"], li["span_root"])


_REF = {}


def reference(lat, kind):
    """the items and, per item, the single path's literal voltages, conducting
    mask and spanning count (tol 1e-8, itmax 2500), computed once"""
    if (lat, kind) not in _REF:
        it = items(lat, kind)
        b1, b2 = api.bond_list(*lat)
        vint, mask, nspan = [], [], []
        with api.Context(*lat) as ctx:
            ctx.set_dot_order(L.DOT_LITERAL)
            for i in range(len(it["trial"])):
                li, c, mk = single_fields(ctx, kind, it, i, b1, b2)
                vint.append(c["vint"])
                mask.append(mk)
                nspan.append(li["nspan"])
        _REF[lat, kind] = dict(it, vint=vint, mask=mask, nspan=nspan)
    return _REF[lat, kind]


def check_against_host(o, lat, mask, vint, Va=1.0, g0=1.0, cut=CUT, what=None):
    """a batch record against the host's on these voltages: counts, maximum and
    histogram exactly, the sums within bar 1"""
    want = api.current_stats_host(*lat, mask, vint, Va, g0, cut)
    for k in INT_KEYS:
        assert o[k] == want[k], (k, what, o[k], want[k])
    assert (o["hist"] == want["hist"]).all() and o["hist"].sum() == o["nbonds"], what
    for k in H.SUM_KEYS:
        assert abs(o[k] - want[k]) <= H.bar1(o["nbonds"]) * want[k], (k, what, o[k], want[k])


def is_zero(o):
    return all(o[k] == 0 for k in L.CURRENTS_KEYS[:-1]) and not o["hist"].any()


CASES = ([(lat, kind) for lat in TBC.LATTICES for kind in KINDS] + [(BIG, L.BOND)])
CASE_IDS = ["%d-%dx%d-%d-%s" % (*lat, KIND_NAME[kind]) for lat, kind in CASES]
_LIT = {}


def literal_run(lat, kind, cur):
    """(batch_cond's items, the currents call's items with voltages) under the
    literal order, computed once"""
    if (lat, kind, cur) not in _LIT:
        ref = reference(lat, kind)
        with api.Context(*lat) as ctx:
            ctx.set_dot_order(L.DOT_LITERAL)
            plain = run(ctx, kind, ref, cur_rule=cur)
            got = run(ctx, kind, ref, cur_rule=cur, currents=True, cut=CUT, voltages=True)
        _LIT[lat, kind, cur] = (plain, got)
    return _LIT[lat, kind, cur]


def counting(ref, got, lat):
    """the items that count: solved by the kernel itself"""
    idx = [i for i, o in enumerate(got) if o["status"] == 0 and o["fallback"] == 0 and o["nspan"] == 1]
    assert len(idx) >= (2 if lat == BIG else 20), (lat, len(idx))
    return idx


@pytest.mark.parametrize("cur", CURS, ids=["fortran", "matlab"])
@pytest.mark.parametrize("lat,kind", CASES, ids=CASE_IDS)
def test_literal_order_voltages(lat, kind, cur):
    ref = reference(lat, kind)
    plain, got = literal_run(lat, kind, cur)
    assert len(plain) == len(got) == len(ref["vint"])
    for i, (p, o) in enumerate(zip(plain, got)):
        for k in ITEM_KEYS:
            assert o[k] == p[k], (k, i, o[k], p[k])
    for i in counting(ref, got, lat):
        assert got[i]["vint"].tobytes() == ref["vint"][i].tobytes(), i
        assert got[i]["vint"].any()


@pytest.mark.parametrize("cur", CURS, ids=["fortran", "matlab"])
@pytest.mark.parametrize("lat,kind", CASES, ids=CASE_IDS)
def test_literal_order_records(lat, kind, cur):
    ref = reference(lat, kind)
    _, got = literal_run(lat, kind, cur)
    for i in counting(ref, got, lat):
        check_against_host(got[i], lat, ref["mask"][i], got[i]["vint"], what=i)
        assert got[i]["nbonds"] > 0 and got[i]["imax"] > 0.0 and 0 < got[i]["nabove"] <= got[i]["nbonds"]
    for i, o in enumerate(got):
        if ref["nspan"][i] == 0:
            assert o["status"] == 1 and is_zero(o) and not o["vint"].any(), i


@pytest.mark.parametrize("lat,kind", CASES, ids=CASE_IDS)
def test_fast_order_records(lat, kind):
    ref = reference(lat, kind)
    with api.Context(*lat) as ctx:
        got = run(ctx, kind, ref, currents=True, cut=CUT, voltages=True)
    for i in counting(ref, got, lat):
        check_against_host(got[i], lat, ref["mask"][i], got[i]["vint"], what=i)


def same_record(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def test_fast_order_deterministic_and_position_independent():
    lat = (0, 50, 50, 0)
    r = TBC.reference(lat, L.SITE)
    it, ns = TBC.fast_grid(r)
    with api.Context(*lat) as ctx:
        kw = dict(site_orders=r["so"], item_nsites=ns, tol=TOL, itmax=ITMAX, currents=True, cut=CUT, voltages=True)
        a = ctx.batch_cond(L.SITE, it, **kw)
        b = ctx.batch_cond(L.SITE, it, **kw)
    assert all(same_record(x, y) for x, y in zip(a, b))  # two runs: bitwise
    assert same_record(a[0], a[299]) and a[0]["status"] == 0 and a[0]["nbonds"] > 0


@pytest.mark.parametrize("order", [L.DOT_LITERAL, L.DOT_FAST], ids=["literal", "fast"])
def test_optional_voltages(order):
    lat, kind = (1, 12, 10, 1), L.SITEBOND
    it = items(lat, kind)
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(order)
        a = run(ctx, kind, it, currents=True, cut=CUT, voltages=True)
        b = run(ctx, kind, it, currents=True, cut=CUT)
    assert any(o["nbonds"] > 0 for o in b)
    for x, y in zip(a, b):
        assert "vint" not in y and all(np.array_equal(x[k], y[k]) for k in y)


def test_chunking_with_voltages():
    """10 x 10: a launch takes at most 16384 items; 16400 items with voltages
    cross the boundary, and the rows on both sides of it are those of
    item-by-item calls"""
    lat, kind = (0, 10, 10, 0), L.BOND
    it = items(lat, kind)
    n0 = len(it["trial"])
    rep = np.arange(16400) % n0
    with api.Context(*lat) as ctx:
        got = run(ctx, kind, it, sel=rep, currents=True, cut=CUT, voltages=True)
        assert len(got) == 16400
        near = list(range(16380, 16400)) + [0, 1, 8191]
        for i in near:
            one = run(ctx, kind, it, sel=rep[i:i + 1], currents=True, cut=CUT, voltages=True)[0]
            assert same_record(got[i], one), i
        assert any(got[i]["nbonds"] > 0 for i in range(16384, 16400))
    # the same item wherever it stands
    for i in range(n0, 16400, 997):
        assert same_record(got[i], got[i % n0]), i


def test_forced_fallback():
    """two columns span at once (test_batch_cond's construction): fallback = 1
    and the record of the host path"""
    m = n = 8
    t = m * n
    lat = (0, m, n, 0)
    c0, c7 = TBC.column_sites(m, n, 0), TBC.column_sites(m, n, 7)
    rest = [k for k in range(1, t + 1) if k not in c0 and k not in c7]
    order = np.array(c0 + c7 + rest + [0], np.int32)
    b1, b2 = api.bond_list(*lat)
    it = dict(so=order[None, :], bo=None, trial=np.array([0], np.int32), ns=np.array([16], np.int32), nb=None)
    with api.Context(*lat) as ctx:
        o = run(ctx, L.SITE, it, currents=True, cut=CUT, voltages=True)[0]
        p = run(ctx, L.SITE, it)[0]
        li, c, mask = single_fields(ctx, L.SITE, it, 0, b1, b2)
    assert o["nspan"] == li["nspan"] == 2 and o["fallback"] == 1
    for k in ITEM_KEYS:
        assert o[k] == p[k], (k, o[k], p[k])
    assert o["vint"].tobytes() == c["vint"].tobytes()
    want = api.current_stats_host(*lat, mask, c["vint"], 1.0, 1.0, CUT)
    assert same_record({k: o[k] for k in L.CURRENTS_KEYS}, want)
    # one column of 8 sites: 7 bonds, the same current in each
    assert o["nbonds"] == 7 and o["nabove"] == 7 and abs(o["imax"] - 1.0 / 7) < 1e-6


def test_no_spanning_cluster_is_zero():
    lat, kind = (0, 10, 10, 0), L.BOND
    it = items(lat, kind)
    sel = np.nonzero(it["nb"] <= 1)[0]
    assert len(sel) >= 2
    with api.Context(*lat) as ctx:
        for o in run(ctx, kind, it, sel=sel, currents=True, cut=CUT, voltages=True):
            assert o["nspan"] == 0 and o["status"] == 1 and is_zero(o) and not o["vint"].any()


@pytest.mark.parametrize("kind", KINDS, ids=KIND_NAME.get)
def test_seeded_call(kind):
    lat = (0, 10, 10, 1)
    it = items(lat, kind)
    ss = api.trial_seeds(58302 if kind != L.SITEBOND else 143285, 3) if kind != L.BOND else None
    bs = api.trial_seeds(58302 if kind == L.BOND else 43716, 3) if kind != L.SITE else None
    with api.Context(*lat) as ctx:
        a = run(ctx, kind, it, currents=True, cut=CUT, voltages=True)
        b = ctx.batch_cond(kind, it["trial"], site_seeds=ss, bond_seeds=bs, item_nsites=it["ns"],
                           item_nbonds=it["nb"], tol=TOL, itmax=ITMAX, currents=True, cut=CUT, voltages=True)
    assert len(a) == len(b) and any(o["nbonds"] > 0 for o in a)
    for i, (x, y) in enumerate(zip(a, b)):
        assert same_record(x, y), i


@pytest.mark.parametrize("vals", R.NONUNIT, ids=["leak-dropped", "leak-kept"])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_NAME.get)
def test_nonunit_values(kind, vals):
    lat = (1, 12, 10, 1)
    Va, g0, leak = vals
    it = items(lat, kind)
    b1, b2 = api.bond_list(*lat)
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        got = run(ctx, kind, it, currents=True, cut=CUT, voltages=True, Va=Va, g0=g0, leak=leak)
        plain = run(ctx, kind, it, Va=Va, g0=g0, leak=leak)
        idx = [i for i, o in enumerate(got) if o["status"] == 0 and o["fallback"] == 0 and o["nspan"] == 1]
        assert len(idx) >= 20
        for i, (p, o) in enumerate(zip(plain, got)):
            for k in ITEM_KEYS:
                assert o[k] == p[k], (k, i)
        for i in idx[::3]:
            li, c, mask = single_fields(ctx, kind, it, i, b1, b2, Va, g0, leak)
            assert got[i]["vint"].tobytes() == c["vint"].tobytes(), i
            check_against_host(got[i], lat, mask, got[i]["vint"], Va, g0, what=i)
            assert got[i]["imax"] <= g0 * Va * (1 + 1e-6)


def test_cut_edge_values():
    lat, kind = (0, 10, 10, 0), L.SITE
    ref = reference(lat, kind)
    with api.Context(*lat) as ctx:
        zero = run(ctx, kind, ref, currents=True, cut=0.0)
        one = run(ctx, kind, ref, currents=True, cut=1.0, voltages=True)
    seen = 0
    for i, (z, o) in enumerate(zip(zero, one)):
        assert z["nabove"] == z["nbonds"] == o["nbonds"]
        if o["status"] == 0 and o["fallback"] == 0 and o["nbonds"]:
            a = H.restate(lat, ref["mask"][i], o["vint"], 1.0, 1.0, 1.0)[0]
            assert o["nabove"] == np.count_nonzero(a == a.max()) >= 1, i
            seen += 1
    assert seen >= 20


def test_current_curve_batched_equals_unbatched():
    lat = (0, 10, 10, 0)
    cases = [(L.BOND, [0.5, 0.6, 0.8], 58302), (L.SITE, [0.6, 0.7, 0.9], 58302),
             (L.SITEBOND, [(0.8, 0.7), (0.9, 0.9), (1.0, 0.6)], 8811064)]
    for kind, grid, master in cases:
        res = {}
        for batch in (True, False):
            with api.Context(*lat) as ctx:
                ctx.set_dot_order(L.DOT_LITERAL)
                res[batch] = api.current_curve(*lat, kind=kind, grid=grid, master=master, numtrials=4, cut=CUT,
                                               batch=batch, ctx=ctx)
        (ra, ca), (rb, cb) = res[True], res[False]
        assert len(ra) == len(rb) == 3 and len(ca) == len(cb) == 4
        nb_max = 0
        for ta, tb in zip(ca, cb):
            for x, y in zip(ta, tb):
                for k in ("gtop", "gbot", "iter", "nspan") + INT_KEYS:
                    assert x[k] == y[k], (k, x[k], y[k])
                assert (x["hist"] == y["hist"]).all()
                for k in H.SUM_KEYS:
                    assert abs(x[k] - y[k]) <= H.bar1(x["nbonds"]) * y[k]
                nb_max = max(nb_max, x["nbonds"])
        for x, y in zip(ra, rb):
            assert x["nspan"] == y["nspan"] and x["G"] == y["G"] and x["backbone"] == y["backbone"]
            assert x["imax"] == y["imax"] and (x["hist"] == y["hist"]).all()
            for k in ("m2", "m4", "m6"):  # means of quotients of sums within bar 1, two roundings more each
                assert abs(x[k] - y[k]) <= (H.bar1(nb_max) + 4 * 2.0 ** -52) * y[k], (k, x[k], y[k])
        assert any(x["nspan"] for x in ra) and sum(int(x["hist"].sum()) for x in ra) > 0
    # seeds in place of orders: the same curve
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        rs, _ = api.current_curve(*lat, kind=L.BOND, grid=[0.5, 0.6, 0.8], master=58302, numtrials=4, cut=CUT,
                                  device_shuffle=True, ctx=ctx)
        ro, _ = api.current_curve(*lat, kind=L.BOND, grid=[0.5, 0.6, 0.8], master=58302, numtrials=4, cut=CUT,
                                  ctx=ctx)
    assert all(same_record(x, y) for x, y in zip(rs, ro))


def test_errors_are_einval():
    with api.Context(0, 91, 93, 0) as ctx:  # no lattice of the default kernel, large flag or not
        so = api.shuffled_ids(ctx.t, 1)
        for large in (False, True):
            ctx.set_batch_large(large)
            with pytest.raises(L.PercError, match="PERC_EINVAL"):
                ctx.batch_cond(L.SITE, [0], site_orders=so, item_nsites=[ctx.t // 2], currents=True)
            assert "perc_batch_currents_supported" in L.lib().perc_last_error().decode()
    with api.Context(0, 10, 10, 0) as ctx:
        t, nb = ctx.t, ctx.nb
        so, bo = api.shuffled_ids(t, 1), api.shuffled_ids(nb, 2)
        site = dict(site_orders=so, item_nsites=[70], currents=True)
        mixed = dict(site_orders=so, bond_orders=bo, item_nsites=[90], item_nbonds=[180], currents=True)
        # the large flag is not read: the default kernel runs
        ctx.set_batch_large(True)
        ok = ctx.batch_cond(L.SITE, [0], **site)
        ctx.set_batch_large(False)
        assert len(ok) == 1 and same_record(ok[0], ctx.batch_cond(L.SITE, [0], **site)[0])
        bad = [
            (L.SITE, [0], dict(site, rule=L.RULE_BOND)),          # perc_batch_cond's cases
            (L.SITEBOND, [0], dict(mixed, rule=L.RULE_SITE)),
            (L.BOND, [0], dict(bond_orders=bo, item_nbonds=[5], rule=L.RULE_SITE, currents=True)),
            (L.BONDSITE, [0], dict(mixed, rule=L.RULE_MIXED)),
            (L.SITE, [0], dict(site, cur_rule=2)),
            (L.SITE, [0], dict(site, cur_rule=-1)),
            (L.SITE, [0], dict(site, itol=3)),
            (L.SITE, [0], dict(site, itol=4)),
            (L.SITE, [0], dict(site, itmax=-1)),
            (L.SITE, [0], dict(item_nsites=[5], currents=True)),
            (L.SITEBOND, [0], dict(site_orders=so, item_nsites=[5], item_nbonds=[5], currents=True)),
            (L.BOND, [0], dict(item_nbonds=[5], currents=True)),
            (L.SITE, [0], dict(site_orders=so, currents=True)),
            (L.SITEBOND, [0], dict(site_orders=so, bond_orders=bo, item_nsites=[5], currents=True)),
            (L.BOND, [0], dict(bond_orders=bo, currents=True)),
            (L.SITE, [1], site),
            (L.SITE, [-1], site),
            (L.SITE, [0], dict(site, item_nsites=[t + 2])),
            (L.SITE, [0], dict(site, item_nsites=[-1])),
            (L.SITEBOND, [0], dict(mixed, item_nbonds=[nb + 2])),
            (L.SITEBOND, [0], dict(mixed, item_nbonds=[-1])),
            (L.BOND, [0], dict(bond_orders=bo, item_nbonds=[nb + 2], currents=True)),
            (L.SITE, [0], dict(site, cut=-1e-9)),                 # cut
            (L.SITE, [0], dict(site, cut=1.0 + 1e-9)),
            (L.SITE, [0], dict(site, cut=float("nan"))),
        ]
        for kind, tr, kw in bad:
            with pytest.raises(L.PercError, match="PERC_EINVAL"):
                ctx.batch_cond(kind, tr, **kw)
            assert L.lib().perc_last_error().decode().startswith("perc_batch_cond_currents:"), (kind, tr, kw)
        with pytest.raises(L.PercError, match="PERC_EINVAL"):  # the seeded call's own text
            ctx.batch_cond(L.SITE, [0], site_seeds=[5], item_nsites=[70], currents=True, cut=2.0)
        assert L.lib().perc_last_error().decode().startswith("perc_batch_cond_currents_seeded:")
        # cur == NULL, ntrials or nitems below 0 (the C entry itself); an empty call is PERC_OK
        lib = L.lib()
        one = np.full(1, 70, np.int32)
        zero = np.zeros(1, np.int32)
        out = (L.BatchItem * 1)()
        cur = np.zeros(1, dtype=L.CURRENTS_DTYPE)

        def call(ntrials, nitems, cur=cur):
            return lib.perc_batch_cond_currents(ctx.h, L.SITE, L.RULE_SITE, L.CUR_MATLAB, ntrials, L.ptr(so), None,
                                                nitems, L.ptr(zero), L.ptr(one), None, 1.0, 1.0, api.LEAK, 2, TOL,
                                                ITMAX, C.cast(out, C.c_void_p), CUT, L.ptr(cur), None)

        assert call(1, 1) == L.PERC_OK
        assert call(1, 1, cur=None) == -1
        assert lib.perc_last_error().decode().startswith("perc_batch_cond_currents: cur")
        assert call(-1, 0) == -1 and call(1, -1) == -1
        assert call(1, 0) == L.PERC_OK and call(0, 0) == L.PERC_OK
        assert ctx.batch_cond(L.SITE, [], site_orders=so, item_nsites=[], currents=True) == []
        # combinations the Python layer refuses
        w = np.ones((1, nb))
        for kw in (dict(weights=w, item_wset=[0]), dict(item_wseed=[1]), dict(solve=False)):
            with pytest.raises(ValueError):
                ctx.batch_cond(L.BOND, [0], bond_orders=bo, item_nbonds=[150], currents=True, **kw)
        with pytest.raises(ValueError):
            ctx.batch_cond(L.BOND, [0], bond_orders=bo, item_nbonds=[150], voltages=True)
