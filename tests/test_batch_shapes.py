"""The one-workgroup batch kernels at the edges of the lattices their support
predicates accept (tests/batch_shapes.py: one interior row, m beyond the
workgroup, 2m > N, m = 3 and 4, the workgroup-size boundaries, arenas the
labeling view limits, the large kernel's and the scan's caps in both extreme
aspects), each held to a reference that does not share the kernel's code:

* k_batch_cond, k_batch_cond_large (forced) and k_batch_cond_w (explicit
  non-unit weights) in the literal dot order: every header field and iter, err,
  gtop, gbot bitwise the single path's (perc_occupy / perc_label /
  perc_conductance) on the same occupancy, all three kinds; on the shapes with
  N <= 300, on 4096 x 3 and on 256 x 64 bitwise the oracle's own assembly +
  literal linbcg + currents as well; non-unit Va / g0 / leak with the leak
  above the 1e-10 threshold where a row touches both electrodes;
* the fast order: test_batch.check_accuracy's bar against the literal result,
  deterministic over two launches and over the item's place;
* the FIELDS epilogue: voltages bitwise the single path's, the record the
  host's (perc_current_stats_host), nbonds the conducting bonds with an
  interior end counted in numpy;
* PERC_BATCH_THREADS = 256 | 512 | 1024 at N = 2048: bitwise one result in the
  literal order; in the fast order the default launch is the workgroup size
  batch_threads' rule names, on both sides of both boundaries;
* k_batch_scan and k_batch_clusters up to t = 16383 flat and thin: records and
  histogram rows api.cluster_stats_host's, first spanning counts the host
  bisection's, order lists and seeds;
* every refused neighbour PERC_EINVAL from the call itself.

The solves of the thin shapes (batch_shapes.LONG) stop at itmax = 300: an
itmax stop is bitwise in the literal order.  Their fast-order results are
checked for determinism only -- check_accuracy's bar is about converged
solves.  The items are batch_shapes.select's; the single path's reference of a
(shape, kind, values) is computed once and shared."""
import ctypes as C

import numpy as np
import pytest

import batch_shapes as BS
import rule_systems as R
import oracle_lib as O
import test_batch as TB
import test_batch_clusters as TCL
import test_batch_currents as TCU
import test_batch_scan as TS
import test_batch_weighted as TW
from percolation_amd import _lib as L
from percolation_amd import api

pytestmark = pytest.mark.gpu
TOL, ITMAX = 1e-8, 20000
TIGHT = 1e-13
CUT = TCU.CUT
UNIT = (1.0, 1.0, api.LEAK)
CURS = [L.CUR_FORTRAN, L.CUR_MATLAB]
NAMES = ("single", "full", "spill", "none", "multi")
HEADER = TB.LABEL_KEYS
COND = TB.COND_KEYS

MID = [(0, 3, 100, 0), (1, 4, 64, 1), (0, 300, 3, 0), (0, 4096, 3, 0), (1, 2048, 3, 1), (0, 2048, 4, 0),
       (0, 4500, 3, 0), (0, 64, 34, 0), (0, 64, 35, 0), (0, 64, 66, 0), (0, 64, 67, 0), (0, 3, 2732, 0)]
SHAPES = {
    "default": BS.TINY + MID,
    "large": BS.TINY + MID + [(0, 3, 2733, 0), (0, 256, 64, 0), (0, 1024, 16, 0), (0, 3, 5461, 0), (1, 4, 4096, 1)],
    "weighted": BS.TINY + [(0, 3, 100, 0), (1, 4, 64, 1), (0, 300, 3, 0), (0, 64, 34, 0), (0, 64, 35, 0),
                           (0, 50, 71, 0), (1, 50, 51, 0)],
}
FAMILY = {"default": "cond", "large": "large", "weighted": "weighted"}
BOTH_RULES = [(0, 4096, 3, 0), (0, 3, 3, 0)]
LEAK_KEPT_SHAPES = [(0, 3, 3, 0), (0, 4096, 3, 0)]
ORACLE = [lat for lat in BS.TINY + MID if BS.sizes(lat)[0] <= 300] + [(0, 4096, 3, 0), (0, 256, 64, 0)]
SCAN_SHAPES = BS.TINY + [(0, 3, 100, 0), (1, 4, 64, 1), (0, 3, 5461, 0), (0, 5461, 3, 0), (0, 4096, 4, 0),
                         (0, 256, 64, 0)]


def cases(path):
    return [(lat, k) for lat in SHAPES[path] for k in BS.supported(FAMILY[path], lat)]


def case_ids(cs):
    return ["%s-%s" % (BS.lat_id(lat), BS.KIND_NAME[k]) for lat, k in cs]


def itmax_of(lat):
    return BS.ITMAX_STOP if lat in BS.LONG else ITMAX


def curs_of(lat, kind):
    return CURS if lat in BOTH_RULES else [api.natural_cur_rule(kind)]


def items_of(lat, kind):
    sel = BS.select(lat, kind)
    names = [n for n in NAMES if n in sel]
    return names, [sel[n] for n in names]


_W = {}


def weights(lat):
    """one row of per-bond multipliers in (0.25, 1.25): no unit, no power of two"""
    if lat not in _W:
        _W[lat] = 0.25 + np.random.RandomState(4100 + lat[1] + 7 * lat[2]).random_sample(BS.sizes(lat)[2])
        _W[lat].setflags(write=False)
    return _W[lat]


_REF = {}


def reference(lat, kind, vals=UNIT, tol=TOL, itmax=None, weighted=False):
    """the single path in the literal order on batch_shapes.select's items:
    per item dict(label, cond[cur_rule], vint, mask), computed once"""
    itmax = itmax_of(lat) if itmax is None else itmax
    key = (lat, kind, vals, tol, itmax, weighted)
    if key in _REF:
        return _REF[key]
    names, items = items_of(lat, kind)
    so, bo = BS.orders(lat)
    b1, b2 = api.bond_list(*lat)
    rule = api.KIND_RULE[kind]
    Va, g0, leak = vals
    ref = []
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        for ns, nbc in items:
            TW.occupy(ctx, kind, so[None, :], bo[None, :], (0, ns, nbc))
            li = ctx.label(canon=True)
            if weighted:
                ctx.set_bond_weights(weights(lat))
            c = ctx.conductance(rule, L.CUR_MATLAB, Va, g0, leak, 2, tol, itmax, vint=True)
            f = dict(c)
            if c["status"] == 0:  # the other rule's currents of the same voltages
                res = L.CondResult()
                L.check(L.lib().perc_currents(ctx.h, rule, L.CUR_FORTRAN, Va, g0, leak, C.byref(res)), "perc_currents")
                f["gtop"], f["gbot"] = res.gtop, res.gbot
            if weighted:
                ctx.set_bond_weights(None)
            socc, bocc = ctx.occupancy()
            mask = api.conducting_bonds(kind, b1, b2, socc, bocc, li["canon"], li["span_root"])
            ref.append(dict(label=li, cond={L.CUR_MATLAB: c, L.CUR_FORTRAN: f}, vint=c["vint"], mask=mask))
    _REF[key] = (names, items, ref)
    return _REF[key]


def launch(ctx, path, lat, kind, items, **kw):
    """one batch_cond call over the items on the path's kernel"""
    ctx.set_batch_large(path == "large")
    if path == "weighted":
        kw.update(weights=weights(lat), item_wset=[0] * len(items))
    return ctx.batch_cond(kind, [0] * len(items), **BS.batch_kw(lat, kind, items), **kw)


def check_items(out, names, ref, cur, what):
    """header and conductance fields of a literal launch against the single
    path; the single-spanning items are solved by the kernel itself"""
    assert len(out) == len(ref) == len(names) >= 3
    for o, name, r in zip(out, names, ref):
        li, c = r["label"], r["cond"][cur]
        w = what + (name, o, li, c)
        for k in HEADER:
            assert o[k] == li[k], (k,) + w
        assert o["fallback"] == (1 if li["nspan"] > 1 else 0), w
        for k in COND:
            assert o[k] == c[k], (k,) + w
        if name in ("single", "full", "spill"):
            assert o["nspan"] == 1 and o["status"] == 0 and o["iter"] > 0 and o["gtop"] > 0.0, w
        elif name == "none":
            assert o["nspan"] == 0 and o["status"] == 1 and o["gtop"] == 0.0 and o["gbot"] == 0.0, w
        else:
            assert o["nspan"] > 1 and o["status"] == 0 and o["gtop"] > 0.0, w


def oracle_of(lat, kind, item, vals, tol, w=None):
    """rule_systems.oracle_conductance on one item's occupancy: the host
    replay's labels, the oracle's bond values (times w), assembly, literal
    linbcg and currents"""
    so, bo = BS.orders(lat)
    rule = api.KIND_RULE[kind]
    b1, b2 = api.bond_list(*lat)
    nb = len(b1)
    lab = api.replay_labels(*lat, kind, site_order=so if kind != L.BOND else None, nsites=item[0],
                            bond_order=bo if kind != L.SITE else None, nbond=item[1])
    assert lab["perccln"] > 0
    bl = lab["bond_label"] if lab["bond_label"] is not None else O.i32(nb)
    sl = lab["site_label"] if lab["site_label"] is not None else O.i32(1)
    s = R.System(rule, *lat, *vals)
    gval = O.f64(nb)
    O.lib().or_bond_values(rule, nb, b1, b2, bl, sl, lab["perccln"], s.g0, s.leak, gval)
    if w is not None:
        inc = gval == -s.g0
        gval[inc] = -s.g0 * w[inc]
    return R.oracle_conductance(s, dict(b1=b1, b2=b2, gval=gval), tol)


def check_oracle(out, names, items, lat, kind, vals, tol, cur, itmax, w=None):
    for o, name, item in zip(out, names, items):
        if name not in ("single", "full"):
            continue
        assert o["iter"] <= itmax  # (converged: the oracle runs to the tolerance)
        oc = oracle_of(lat, kind, item, vals, tol, w)
        what = (lat, kind, name, cur, o, oc["iter"], oc["err"], oc["cur"][cur])
        assert o["iter"] == oc["iter"] and o["err"] == oc["err"], what
        assert (o["gtop"], o["gbot"]) == oc["cur"][cur], what


def literal_case(path, lat, kind, vals=UNIT, tol=TOL, curs=None):
    weighted = path == "weighted"
    itmax = itmax_of(lat)
    names, items, ref = reference(lat, kind, vals, tol, weighted=weighted)
    Va, g0, leak = vals
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        for cur in curs or curs_of(lat, kind):
            out = launch(ctx, path, lat, kind, items, cur_rule=cur, Va=Va, g0=g0, leak=leak, tol=tol, itmax=itmax)
            for o, name in zip(out, names):
                print("%s %s %s %s cur %d: nspan %d iter %d err %.3e gtop %.17g gbot %.17g"
                      % (path, BS.lat_id(lat), BS.KIND_NAME[kind], name, cur, o["nspan"], o["iter"], o["err"],
                         o["gtop"], o["gbot"]))
            check_items(out, names, ref, cur, (path, lat, kind, cur))
            if lat in ORACLE:
                check_oracle(out, names, items, lat, kind, vals, tol, cur, itmax, weights(lat) if weighted else None)
    return out


# ---------------------------------------------------------------- conductance, literal order
@pytest.mark.parametrize("lat,kind", cases("default"), ids=case_ids(cases("default")))
def test_default_kernel_literal_bitwise(lat, kind):
    assert api.batch_cond_supported(kind, *lat)
    literal_case("default", lat, kind)


@pytest.mark.parametrize("lat,kind", cases("large"), ids=case_ids(cases("large")))
def test_large_kernel_literal_bitwise(lat, kind):
    assert api.batch_large_supported(kind, *lat)
    literal_case("large", lat, kind)


@pytest.mark.parametrize("lat,kind", cases("weighted"), ids=case_ids(cases("weighted")))
def test_weighted_kernel_literal_bitwise(lat, kind):
    assert api.batch_weighted_supported(kind, *lat)
    out = literal_case("weighted", lat, kind)
    # the weights are read: not the unweighted result
    names, _, plain = reference(lat, kind)
    i = names.index("full")
    assert out[i]["gtop"] != plain[i]["cond"][api.natural_cur_rule(kind)]["gtop"]


@pytest.mark.parametrize("path", ["default", "large"])
@pytest.mark.parametrize("kind", BS.KINDS, ids=BS.KIND_NAME.get)
@pytest.mark.parametrize("lat", LEAK_KEPT_SHAPES, ids=BS.lat_id)
def test_leak_kept_where_a_row_touches_both_electrodes(lat, kind, path):
    """Va = 0.3, g0 = 13, leak = 3e-9: the Fortran rule's `>= 1e-10` branch
    keeps the leak terms of rows with both electrodes as neighbours"""
    assert lat[2] == 3
    literal_case(path, lat, kind, vals=R.LEAK_KEPT, curs=CURS)


@pytest.mark.parametrize("path", ["default", "large", "weighted"])
@pytest.mark.parametrize("kind", BS.KINDS, ids=BS.KIND_NAME.get)
def test_thin_shape_runs_to_both_tolerances(kind, path):
    lat = (0, 3, 100, 0)
    for tol in (TOL, TIGHT):
        out = literal_case(path, lat, kind, tol=tol)
        assert all(o["err"] <= tol and o["iter"] <= ITMAX for o in out if o["nspan"] == 1)


# ---------------------------------------------------------------- the fast order
def solved_items(lat, kind):
    names, items = items_of(lat, kind)
    return [it for n, it in zip(names, items) if n in ("single", "full", "spill")]


FAST_CASES = [(path, lat) for path in ("default", "large", "weighted") for lat in SHAPES[path]]


@pytest.mark.parametrize("path,lat", FAST_CASES, ids=["%s-%s" % (p, BS.lat_id(lat)) for p, lat in FAST_CASES])
def test_fast_order(lat, path):
    """two launches and two places of one item: bitwise; against the literal
    result: 2 trunc + max(1e-10, tol), trunc from a literal run at 1e-13"""
    kinds = BS.supported(FAMILY[path], lat)
    assert kinds
    itmax = itmax_of(lat)
    with api.Context(*lat) as ctx:
        for kind in kinds:
            it = solved_items(lat, kind)
            grid = it + [it[0]]
            ctx.set_dot_order(L.DOT_FAST)
            a = launch(ctx, path, lat, kind, grid, tol=TOL, itmax=itmax)
            b = launch(ctx, path, lat, kind, grid, tol=TOL, itmax=itmax)
            assert a == b and a[0] == a[-1], (lat, kind)
            assert all(o["nspan"] == 1 and o["fallback"] == 0 and o["status"] == 0 and o["iter"] > 0 for o in a)
            if lat in BS.LONG:
                continue
            ctx.set_dot_order(L.DOT_LITERAL)
            lit = launch(ctx, path, lat, kind, it, tol=TOL, itmax=itmax)
            tight = launch(ctx, path, lat, kind, it, tol=TIGHT, itmax=itmax)
            for f, r, tg, item in zip(a, lit, tight, it):
                assert max(f["iter"], r["iter"], tg["iter"]) <= itmax and tg["err"] <= TIGHT, (lat, kind, item, f, r, tg)
                d = TB.check_accuracy(f, r, tg, (lat, kind, item))
                print("%s %s %s %s: rel %.3e (iter %d, literal %d, tight %d)"
                      % (path, BS.lat_id(lat), BS.KIND_NAME[kind], item, d, f["iter"], r["iter"], tg["iter"]))


# ---------------------------------------------------------------- the currents epilogue
CUR_CASES = [(lat, k) for lat in SHAPES["default"] for k in BS.supported("currents", lat)]


@pytest.mark.parametrize("lat,kind", CUR_CASES, ids=case_ids(CUR_CASES))
def test_currents_epilogue(lat, kind):
    names, items, ref = reference(lat, kind)
    N, t, nb = BS.sizes(lat)
    m = lat[1]
    b1, b2 = api.bond_list(*lat)
    interior = ((b1 > m) & (b1 <= t - m)) | ((b2 > m) & (b2 <= t - m))
    itmax = itmax_of(lat)
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        kw = dict(BS.batch_kw(lat, kind, items), tol=TOL, itmax=itmax)
        plain = ctx.batch_cond(kind, [0] * len(items), **kw)
        got = ctx.batch_cond(kind, [0] * len(items), currents=True, cut=CUT, voltages=True, **kw)
    for o, p, name, r in zip(got, plain, names, ref):
        what = (lat, kind, name)
        for k in TCU.ITEM_KEYS:
            assert o[k] == p[k], (k,) + what
        if name == "none":
            assert o["status"] == 1 and TCU.is_zero(o) and not o["vint"].any(), what
            continue
        assert o["vint"].shape == (N,) and o["vint"].tobytes() == r["vint"].tobytes(), what
        assert o["vint"].any()
        # (a multi item is the host path's record of the same voltages)
        TCU.check_against_host(o, lat, r["mask"], o["vint"], what=what)
        # the record's bonds: the conducting ones with an interior end (at n = 3: with an end in the one row)
        assert o["nbonds"] == np.count_nonzero(r["mask"].astype(bool) & interior) > 0, what
        assert o["imax"] > 0.0 and 0 < o["nabove"] <= o["nbonds"], what


# ---------------------------------------------------------------- the workgroup size
def test_threads_override_literal_bitwise(monkeypatch):
    """N = 2048 fits 256, 512 and 1024 threads: one literal result; at
    N = 2112 a request for 256 does not fit and is ignored"""
    lat, kind = (0, 64, 34, 0), L.BOND
    names, items, ref = reference(lat, kind)
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        for nt in ("256", "512", "1024"):
            monkeypatch.setenv("PERC_BATCH_THREADS", nt)
            out = launch(ctx, "default", lat, kind, items, tol=TOL, itmax=ITMAX)
            check_items(out, names, ref, L.CUR_FORTRAN, (lat, nt))
    lat = (0, 64, 35, 0)
    names, items, ref = reference(lat, kind)
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        monkeypatch.setenv("PERC_BATCH_THREADS", "256")
        out = launch(ctx, "default", lat, kind, items, tol=TOL, itmax=ITMAX)
        check_items(out, names, ref, L.CUR_FORTRAN, (lat, "256 ignored"))


@pytest.mark.parametrize("lat,want", [((0, 64, 34, 0), 256), ((0, 64, 35, 0), 512), ((0, 64, 66, 0), 512),
                                      ((0, 64, 67, 0), 1024)], ids=lambda v: BS.lat_id(v) if isinstance(v, tuple) else str(v))
def test_default_workgroup_size_is_the_rules(lat, want, monkeypatch):
    """The fast order's sums follow the workgroup size (a thread's rows, then
    the waves), so the default launch is bitwise the launch under
    PERC_BATCH_THREADS = the size the rule names (the fewest threads at
    kBatchEPT = 8 rows each) and, on these items, not the next size's; a
    size that does not fit is ignored."""
    N = BS.sizes(lat)[0]
    assert want == next(nt for nt in (256, 512, 1024) if 8 * nt >= N)
    kind = L.SITE
    it = solved_items(lat, kind)
    res = {}
    with api.Context(*lat) as ctx:
        for nt in (None, 256, 512, 1024):
            if nt is None:
                monkeypatch.delenv("PERC_BATCH_THREADS", raising=False)
            else:
                monkeypatch.setenv("PERC_BATCH_THREADS", str(nt))
            res[nt] = launch(ctx, "default", lat, kind, it, tol=TOL, itmax=itmax_of(lat))
    assert all(o["status"] == 0 and o["iter"] > 1 for o in res[None])
    assert res[None] == res[want]
    for nt in (256, 512):
        if nt < want:
            assert res[nt] == res[None], nt  # does not fit: ignored
    if want < 1024:
        assert res[2 * want] != res[None]  # the comparison can tell the sizes apart


# ---------------------------------------------------------------- scan and clusters
def trial_orders(lat):
    """three trials per list: the shape's own orders first"""
    _, t, nb = BS.sizes(lat)
    seeds = np.array([BS.SEED, BS.SEED + 2, BS.SEED + 4], np.int32)
    so = np.stack([api.shuffled_ids(t, int(s)) for s in seeds])
    bo = np.stack([api.shuffled_ids(nb, int(s) + 1) for s in seeds])
    return seeds, seeds + 1, so, bo


@pytest.mark.parametrize("kind", BS.KINDS, ids=BS.KIND_NAME.get)
@pytest.mark.parametrize("lat", SCAN_SHAPES, ids=BS.lat_id)
def test_clusters_exact(lat, kind):
    assert api.batch_clusters_supported(*lat, TCL.NMAX)
    names, items = items_of(lat, kind)
    # the empty lattice and one element besides
    items = items + [(0, 0), (1 if kind != L.BOND else 0, 1 if kind != L.SITE else 0)]
    so, bo = BS.orders(lat)
    want = [TCL.host(lat, kind, so, ns, bo, nbc) for ns, nbc in items]
    assert [int(w[0]["nspan"]) for w in want[:2]] == [1, 1]
    kw = BS.batch_kw(lat, kind, items)
    skw = {k.replace("orders", "seeds"): ([BS.SEED] if k == "site_orders" else [BS.SEED + 1] if k == "bond_orders"
                                         else v) for k, v in kw.items()}
    with api.Context(*lat) as ctx:
        for nexact in (0, 12, TCL.NMAX):
            recs, hist = ctx.batch_clusters(kind, [0] * len(items), nexact=nexact, **kw)
            assert hist.shape == (len(items), nexact + 32)
            TCL.check(recs, hist, want, nexact, (lat, kind, nexact))
        recs, hist = ctx.batch_clusters(kind, [0] * len(items), nexact=12, **skw)
        TCL.check(recs, hist, want, 12, (lat, kind, "seeded"))


@pytest.mark.parametrize("kind", BS.KINDS, ids=BS.KIND_NAME.get)
@pytest.mark.parametrize("lat", SCAN_SHAPES, ids=BS.lat_id)
def test_scan_first_spanning(lat, kind):
    """bond and site: the single path's bisection and sizes
    (test_batch_scan.single); mixed: bonds scanned over the sites of the
    shape's partial item (perc_first_spanning_mixed); every first count also
    against the host's labels -- it spans, one entry fewer does not"""
    assert api.scan_supported(*lat)
    _, t, nb = BS.sizes(lat)
    sseeds, bseeds, so, bo = trial_orders(lat)
    with api.Context(*lat) as ctx:
        if kind == L.SITEBOND:
            fixed = BS.select(lat, kind)["single"][0]
            got = ctx.batch_scan(kind, site_orders=so, bond_orders=bo, scan=L.BOND, fixed=fixed)
            seeded = ctx.batch_scan_seeded(kind, site_seeds=sseeds, bond_seeds=bseeds, scan=L.BOND, fixed=fixed)
            want = [api.first_spanning_mixed(ctx, L.BOND, so[i], fixed, bo[i], nb) for i in range(3)]
            assert [g["first"] for g in got] == want
            assert got[0]["first"] > 0
        else:
            orders = bo if kind == L.BOND else so
            got = ctx.batch_scan(kind, **TS.orders_kw(kind, orders))
            seeded = ctx.batch_scan_seeded(kind, **{"bond_seeds" if kind == L.BOND else "site_seeds":
                                                    bseeds if kind == L.BOND else sseeds})
            want = [TS.single(ctx, o, kind) for o in orders]
            TS.check_items(got, want, (lat, kind))
            assert all(g["first"] > 0 for g in got)
    assert seeded == got
    print("%s %s: first %s" % (BS.lat_id(lat), BS.KIND_NAME[kind], [g["first"] for g in got]))
    for i, g in enumerate(got):
        c = g["first"]
        if c == 0:
            continue
        at = (fixed, c) if kind == L.SITEBOND else ((0, c) if kind == L.BOND else (c, 0))
        below = (fixed, c - 1) if kind == L.SITEBOND else ((0, c - 1) if kind == L.BOND else (c - 1, 0))
        assert api.cluster_stats_host(*lat, kind, so[i], at[0], bo[i], at[1], 0)[0]["nspan"] >= 1, (i, c)
        assert api.cluster_stats_host(*lat, kind, so[i], below[0], bo[i], below[1], 0)[0]["nspan"] == 0, (i, c)


# ---------------------------------------------------------------- refusals
def einval(f, *a, **kw):
    with pytest.raises(L.PercError, match="PERC_EINVAL"):
        f(*a, **kw)


def test_refused_neighbours_are_einval_from_the_call():
    for lat, kinds in (((0, 4500, 3, 0), (L.SITE, L.SITEBOND)), ((0, 3, 2733, 0), BS.KINDS)):
        with api.Context(*lat) as ctx:
            for kind in kinds:  # the default kernel and its currents epilogue
                assert not api.batch_cond_supported(kind, *lat)
                kw = BS.batch_kw(lat, kind, [BS.select(lat, kind)["full"]])
                einval(ctx.batch_cond, kind, [0], **kw)
                einval(ctx.batch_cond, kind, [0], currents=True, **kw)
            if lat == (0, 3, 2733, 0):
                einval(ctx.batch_bondc, BS.orders(lat)[1], [0], [BS.sizes(lat)[2]])
            else:  # the bond kind is taken
                o = ctx.batch_cond(L.BOND, [0], solve=False, **BS.batch_kw(lat, L.BOND, [BS.select(lat, L.BOND)["full"]]))
                assert o[0]["nspan"] == 1
    for lat in ((0, 50, 72, 0), (1, 50, 52, 0), (0, 4096, 3, 0)):  # the weighted kernel
        with api.Context(*lat) as ctx:
            for kind in BS.KINDS:
                assert not api.batch_weighted_supported(kind, *lat)
                kw = BS.batch_kw(lat, kind, [BS.select(lat, kind)["full"]])
                einval(ctx.batch_cond, kind, [0], weights=weights(lat), item_wset=[0], **kw)
                einval(ctx.batch_cond, kind, [0], item_wseed=[5], **kw)
    for lat in ((0, 5461, 3, 0), (0, 4096, 4, 0)):  # the large kernel, forced
        with api.Context(*lat) as ctx:
            ctx.set_batch_large(True)
            for kind in BS.KINDS:
                assert not api.batch_large_supported(kind, *lat)
                einval(ctx.batch_cond, kind, [0], **BS.batch_kw(lat, kind, [BS.select(lat, kind)["full"]]))
    lat = (0, 3, 5462, 0)  # the scan and the cluster kernels
    _, t, nb = BS.sizes(lat)
    so, bo = BS.orders(lat)
    with api.Context(*lat) as ctx:
        einval(ctx.batch_scan, L.BOND, bond_orders=bo)
        einval(ctx.batch_scan, L.SITE, site_orders=so)
        einval(ctx.batch_scan, L.SITEBOND, site_orders=so, bond_orders=bo, scan=L.BOND, fixed=t)
        einval(ctx.batch_scan_seeded, L.SITE, site_seeds=[BS.SEED])
        einval(ctx.batch_clusters, L.BOND, [0], bond_orders=bo, item_nbonds=[nb])
        einval(ctx.batch_clusters, L.SITE, [0], site_orders=so, item_nsites=[t])
        einval(ctx.batch_clusters, L.SITEBOND, [0], site_orders=so, bond_orders=bo, item_nsites=[t], item_nbonds=[nb])
        einval(ctx.batch_clusters, L.SITE, [0], site_seeds=[BS.SEED], item_nsites=[t])
        ctx.set_batch_large(True)
        einval(ctx.batch_cond, L.SITE, [0], site_orders=so, item_nsites=[t])
