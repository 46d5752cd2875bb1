"""The large batch kernel (perc_set_batch_large, k_batch_cond_large): the batch
path's one-workgroup realisation with p alone in LDS, the row codes and r in
registers at up to 16 rows per thread and q held there (fast order) or
rebuilt (literal order), for lattices up to 128 x 128.  Opt-in per context.

* forced on the small lattices of test_batch_cond: every item record equal
  to the default batch kernel's, literal order, all three kinds, both
  current rules;
* more than 8 rows per thread (91 x 93, 128 x 128, 64 x 256, the triangular
  128 x 128 pbc lattice's labeling view): the literal order bitwise the
  single path, an itmax stop included;
* the fast order: deterministic, independent of the item's place in the
  grid, within test_batch.check_accuracy's bar;
* the fallback replay, the seeded call, the flag and its PERC_EINVAL cases,
  api.cond_curve(large=True) and Ensemble(large=True).

Every seed below is entry 0 of trial_seeds(58302): on each listed lattice and
occupancy exactly one cluster spans (checked on the host before the first
GPU run; the tests assert it)."""
import ctypes as C

import numpy as np
import pytest

import golden_io as G
import test_batch as TB
import test_batch_cond as TC
from percolation_amd import _lib as L
from percolation_amd import api

pytestmark = pytest.mark.gpu
TOL, ITMAX = 1e-8, 2500
TIGHT, TIGHT_ITMAX = 1e-13, 20000
KINDS = [L.BOND, L.SITE, L.SITEBOND]
KIND_NAME = {L.BOND: "bond", L.SITE: "site", L.SITEBOND: "mixed"}
ITEM_KEYS = ("nclusters", "nspan", "span_root", "span_sites", "fallback", "status", "iter", "err", "gtop", "gbot")
SEED = int(api.trial_seeds(58302, 1)[0])


def small_items(kind, lat):
    """test_batch_cond.items_of's lists; the bond kind: test_batch.reference's
    counts of three trials, as arguments of batch_cond"""
    if kind != L.BOND:
        (ss, bs), it = TC.items_of(kind, lat)
    else:
        nb = api.nbonds(*lat)
        counts = sorted({int(c) for c in api.pb_grid(lat[0], nb) if 0 < c <= nb} | {0, 1, nb, nb + 1})
        ss, bs = None, api.trial_seeds(58302, 3)
        it = [(tr, 0, c) for tr in range(3) for c in counts]
    t, nb = lat[1] * lat[2], api.nbonds(*lat)
    kw = dict(site_orders=None if ss is None else np.stack([api.shuffled_ids(t, int(s)) for s in ss]),
              bond_orders=None if bs is None else np.stack([api.shuffled_ids(nb, int(s)) for s in bs]),
              item_nsites=None if ss is None else [x[1] for x in it],
              item_nbonds=None if bs is None else [x[2] for x in it])
    return [x[0] for x in it], kw


def assert_items_equal(got, want, what):
    assert len(got) == len(want) > 0
    for i, (g, w) in enumerate(zip(got, want)):
        for k in ITEM_KEYS:
            assert g[k] == w[k], (what, i, k, g, w)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_NAME.get)
@pytest.mark.parametrize("lat", TC.LATTICES)
def test_forced_on_small_lattices_equals_default_kernel(lat, kind):
    assert api.batch_cond_supported(kind, *lat) and api.batch_large_supported(kind, *lat)
    it, kw = small_items(kind, lat)
    curs = TC.CURS if lat == (0, 50, 50, 0) else [api.natural_cur_rule(kind)]
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        for cur in curs:
            want = ctx.batch_cond(kind, it, cur_rule=cur, tol=TOL, itmax=ITMAX, **kw)
            ctx.set_batch_large(True)
            got = ctx.batch_cond(kind, it, cur_rule=cur, tol=TOL, itmax=ITMAX, **kw)
            ctx.set_batch_large(False)
            assert_items_equal(got, want, (lat, kind, cur))
            assert any(w["status"] == 0 and w["iter"] > 0 for w in want)
            assert any(w["nspan"] == 0 for w in want)
        if kind == L.BOND:  # perc_batch_bondc takes the flag as well
            want = ctx.batch_bondc(kw["bond_orders"], it, kw["item_nbonds"], tol=TOL, itmax=ITMAX)
            ctx.set_batch_large(True)
            got = ctx.batch_bondc(kw["bond_orders"], it, kw["item_nbonds"], tol=TOL, itmax=ITMAX)
            assert_items_equal(got, want, (lat, "bondc"))


def edge_items(kind, t, nb):
    """two items per kind: (nsites, nbonds)"""
    if kind == L.BOND:
        return [(0, int(0.55 * nb)), (0, nb)]
    if kind == L.SITE:
        return [(int(0.66 * t), 0), (t, 0)]
    return [(int(0.90 * t), int(0.80 * nb)), (t, nb)]


def orders_of(kind, t, nb):
    so = api.shuffled_ids(t, SEED) if kind != L.BOND else None
    bo = api.shuffled_ids(nb, SEED) if kind != L.SITE else None
    return so, bo


def single(ctx, kind, so, ns, bo, nbc, cur, tol=TOL, itmax=ITMAX, solve=True):
    """labels and the conductance record of the single path on one item"""
    if kind == L.BOND:
        ctx.occupy(L.BOND, bond_order=bo, nbonds_=int(nbc))
    else:
        TC.occupy(ctx, kind, so, ns, bo, nbc)
    li = ctx.label()
    c = ctx.conductance(api.KIND_RULE[kind], cur, 1.0, 1.0, api.LEAK, 2, tol, itmax) if solve else None
    return li, c


def large_items(ctx, kind, so, bo, items, **kw):
    return ctx.batch_cond(kind, [0] * len(items), site_orders=so, bond_orders=bo,
                          item_nsites=[x[0] for x in items] if so is not None else None,
                          item_nbonds=[x[1] for x in items] if bo is not None else None, **kw)


def check_bitwise_single(lat, kind, items, itmax=ITMAX):
    """the large kernel in the literal order against perc_conductance under
    PERC_DOT_LITERAL on the same occupancies: every label and conductance
    field; every item spans once and is solved by the kernel"""
    cur = api.natural_cur_rule(kind)
    with api.Context(*lat) as ctx:
        so, bo = orders_of(kind, ctx.t, ctx.nb)
        ctx.set_dot_order(L.DOT_LITERAL)
        ctx.set_batch_large(True)
        out = large_items(ctx, kind, so, bo, items, tol=TOL, itmax=itmax)
        for o, (ns, nbc) in zip(out, items):
            assert o["nspan"] == 1 and o["fallback"] == 0 and o["status"] == 0, (lat, kind, ns, nbc, o)
            li, c = single(ctx, kind, so, ns, bo, nbc, cur, itmax=itmax)
            print("%s %s (%d, %d): iter %d err %.3e gtop %.17g" % (lat, KIND_NAME[kind], ns, nbc, o["iter"],
                                                                  o["err"], o["gtop"]))
            for k in TB.LABEL_KEYS:
                assert o[k] == li[k], (k, ns, nbc, o, li)
            for k in TB.COND_KEYS:
                assert o[k] == c[k], (k, ns, nbc, o, c)
            assert o["iter"] > 0 and o["gtop"] > 0.0
    return out


@pytest.mark.parametrize("kind", KINDS, ids=KIND_NAME.get)
@pytest.mark.parametrize("m,n", [(91, 93), (128, 128), (64, 256)])
def test_more_than_8_rows_per_thread_literal_bitwise(m, n, kind):
    """N = 8281 (a ninth row on 89 threads only), N = 16128 (a ragged
    sixteenth row), t = 16384 (the cap)"""
    lat = (0, m, n, 0)
    assert not api.batch_cond_supported(kind, *lat) and api.batch_large_supported(kind, *lat)
    check_bitwise_single(lat, kind, edge_items(kind, m * n, api.nbonds(*lat)))


def test_largest_labeling_view_literal_bitwise():
    """triangular 128 x 128 pbc, mixed kind: the labeling view overhangs p"""
    lat = (1, 128, 128, 1)
    check_bitwise_single(lat, L.SITEBOND, edge_items(L.SITEBOND, 128 * 128, api.nbonds(*lat)))


def test_itmax_stop_bitwise():
    lat = (0, 128, 128, 0)
    nb = api.nbonds(*lat)
    out = check_bitwise_single(lat, L.BOND, [(0, int(0.55 * nb))], itmax=5)
    assert out[0]["iter"] == 6 and out[0]["err"] > TOL  # (linbcg stops at iter > itmax)


FAST_LAT = (0, 128, 128, 0)


def fast_counts(nb):
    return [int(0.55 * nb), int(0.60 * nb), int(0.70 * nb), nb]


def test_fast_order_deterministic_and_position_independent():
    with api.Context(*FAST_LAT) as ctx:
        nb = ctx.nb
        bo = api.shuffled_ids(nb, SEED)
        ctx.set_batch_large(True)
        four = [(0, c) for c in fast_counts(nb)]
        a = large_items(ctx, L.BOND, None, bo, four, tol=TOL, itmax=ITMAX)
        b = large_items(ctx, L.BOND, None, bo, four, tol=TOL, itmax=ITMAX)
        assert a == b
        assert all(o["nspan"] == 1 and o["fallback"] == 0 and o["status"] == 0 and o["iter"] > 0 for o in a)
        grid = fast_counts(nb)
        forty = [four[0]] + [(0, grid[i % 4]) for i in range(1, 39)] + [four[0]]
        c = large_items(ctx, L.BOND, None, bo, forty, tol=TOL, itmax=ITMAX)
        assert len(c) == 40 and c[0] == c[39] == a[0]
        for i in range(1, 39):
            assert c[i] == a[i % 4], i


def test_fast_order_accuracy():
    """test_batch.check_accuracy's bar, unchanged: the fast result against the
    literal one at the same tol, the truncation term from a literal run at
    1e-13 (the literal order is the one the tests above pin to the single
    path)"""
    with api.Context(*FAST_LAT) as ctx:
        nb = ctx.nb
        bo = api.shuffled_ids(nb, SEED)
        ctx.set_batch_large(True)
        four = [(0, c) for c in fast_counts(nb)]
        fast = large_items(ctx, L.BOND, None, bo, four, tol=TOL, itmax=TIGHT_ITMAX)
        ctx.set_dot_order(L.DOT_LITERAL)
        lit = large_items(ctx, L.BOND, None, bo, four, tol=TOL, itmax=TIGHT_ITMAX)
        tight = large_items(ctx, L.BOND, None, bo, four, tol=TIGHT, itmax=TIGHT_ITMAX)
    for f, r, tg, (_, cnt) in zip(fast, lit, tight, four):
        for o in (f, r, tg):
            assert o["nspan"] == 1 and o["fallback"] == 0 and o["status"] == 0, (cnt, o)
        assert r["iter"] <= TIGHT_ITMAX and tg["iter"] <= TIGHT_ITMAX and tg["err"] <= TIGHT, (cnt, r, tg)
        d = TB.check_accuracy(f, r, tg, cnt)
        print("count %d: rel %.3e (iter %d, literal %d, tight %d)" % (cnt, d, f["iter"], r["iter"], tg["iter"]))


def test_forced_fallback():
    """91 x 93, columns 0 and m - 1 occupied first: two clusters span, the
    item goes through the single path on the context"""
    m, n = 91, 93
    nb = api.nbonds(0, m, n, 0)
    c0, c1 = TB.column_bonds(m, n, 0), TB.column_bonds(m, n, m - 1)
    assert len(c0) == len(c1) == n - 1
    both = set(c0) | set(c1)
    rest = [k for k in range(1, nb + 1) if k not in both]
    order = np.array(c0 + c1 + rest + [0], np.int32)
    count = len(c0) + len(c1)
    with api.Context(0, m, n, 0) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        for solve in (False, True):
            ctx.set_batch_large(True)
            o = ctx.batch_bondc(order, [0], [count], solve=solve, tol=TOL, itmax=ITMAX)[0]
            li, cr = TB.single(ctx, order, count, solve=solve)
            assert o["nspan"] == li["nspan"] == 2 and o["fallback"] == 1
            for k in TB.LABEL_KEYS:
                assert o[k] == li[k], (k, o, li)
            if solve:
                for k in TB.COND_KEYS:
                    assert o[k] == cr[k], (k, o, cr)
                assert o["gtop"] > 0.0


def test_seeded_equals_orders():
    lat = (0, 128, 128, 0)
    with api.Context(*lat) as ctx:
        t = ctx.t
        so = np.zeros(t + 1, np.int32)
        L.lib().perc_shuffle_seeded(SEED, t, so)
        ns = [int(0.66 * t), t]
        ctx.set_batch_large(True)
        want = ctx.batch_cond(L.SITE, [0, 0], site_orders=so, item_nsites=ns, tol=TOL, itmax=ITMAX)
        got = ctx.batch_cond(L.SITE, [0, 0], site_seeds=[SEED], item_nsites=ns, tol=TOL, itmax=ITMAX)
    assert_items_equal(got, want, "seeded")
    assert all(o["nspan"] == 1 and o["status"] == 0 and o["iter"] > 0 for o in want)


def test_flag():
    lib = L.lib()
    with api.Context(0, 91, 93, 0) as ctx:
        order = api.shuffled_ids(ctx.nb, SEED)
        args = (order, [0], [int(0.55 * ctx.nb)])
        assert lib.perc_batch_large(ctx.h) == 0 and ctx.batch_large() is False
        with pytest.raises(L.PercError, match="PERC_EINVAL"):
            ctx.batch_bondc(*args)
        assert "perc_batch_supported" in lib.perc_last_error().decode()
        ctx.set_batch_large()
        assert lib.perc_batch_large(ctx.h) == 1 and ctx.batch_large() is True
        o = ctx.batch_bondc(*args)[0]
        assert o["nspan"] == 1 and o["status"] == 0 and o["iter"] > 0 and o["gtop"] > 0.0
        ctx.set_batch_large(False)
        assert lib.perc_batch_large(ctx.h) == 0
        with pytest.raises(L.PercError, match="PERC_EINVAL"):
            ctx.batch_bondc(*args)
        so = api.shuffled_ids(ctx.t, SEED)
        with pytest.raises(L.PercError, match="PERC_EINVAL"):
            ctx.batch_cond(L.SITE, [0], site_orders=so, item_nsites=[ctx.t // 2])
    assert lib.perc_batch_large(None) == -1 and lib.perc_set_batch_large(None, 1) == -1
    with api.Context(0, 129, 128, 0) as ctx:
        ctx.set_batch_large(True)
        order = api.shuffled_ids(ctx.nb, SEED)
        so = api.shuffled_ids(ctx.t, SEED)
        with pytest.raises(L.PercError, match="PERC_EINVAL"):
            ctx.batch_bondc(order, [0], [ctx.nb // 2])
        assert "perc_batch_large_supported" in lib.perc_last_error().decode()
        for seeded in (False, True):
            src = dict(site_seeds=[SEED]) if seeded else dict(site_orders=so)
            with pytest.raises(L.PercError, match="PERC_EINVAL"):
                ctx.batch_cond(L.SITE, [0], item_nsites=[ctx.t // 2], **src)
            assert "perc_batch_large_supported" in lib.perc_last_error().decode()


def test_cond_curve_large_equals_unbatched():
    lat = (0, 91, 93, 0)
    grid = [0.62, 0.66, 0.80]
    res = {}
    for batch, large in ((64, True), (0, False), (64, False)):
        with api.Context(*lat) as ctx:
            ctx.set_dot_order(L.DOT_LITERAL)
            res[batch, large] = api.cond_curve(*lat, kind=L.SITE, grid=grid, master=58302, numtrials=1,
                                               batch=batch, ctx=ctx, large=large)
            assert ctx.batch_large() is False  # restored
    (ra, sa), (rb, sb) = res[64, True], res[0, False]
    assert ra == rb and len(ra) == 1 and len(ra[0]["rows"]) == 3
    assert sa.tobytes() == sb.tobytes() and (sa[:, 0] == 1).all() and sa[:, 3].any()
    assert any(r["iter"] > 0 and r["gtop"] > 0.0 for r in ra[0]["rows"])
    # large=False on this lattice: the per-item loop, as before
    assert res[64, False][0] == rb and res[64, False][1].tobytes() == sb.tobytes()


def test_ensemble_large_literal_golden():
    v = "sq_bond_cond_3t"
    p = G.meta(v)["params"]
    with api.Ensemble(p["lattice"], p["m"], p["n"], p["pbc"], ndev=1, batch=64, large=True) as e:
        assert e.batch == 64 and e.large is True
        assert L.lib().perc_batch_large(C.c_void_p(L.lib().perc_ensemble_ctx(e.h, 0))) == 1
        e.set_dot_order(L.DOT_LITERAL)
        res, _ = e.bond_cond(p["seed"], p["numtrials"])
    want = TB.golden_trials(v)
    assert len(res) == len(want)
    for tr, w in zip(res, want):
        assert len(tr["rows"]) == len(w["rows"])
        for r, wr in zip(tr["rows"], w["rows"]):
            assert "%12.9f" % r["pb"] == "%12.9f" % wr[0]
            assert abs(r["gbot"] - wr[1]) <= 2e-9 and abs(r["gtop"] - wr[2]) <= 2e-9, (r, wr)
        assert tr["pc"] == w["pc"] and tr["perccln"] == w["perccln"]


def test_ensemble_large_switch():
    with api.Ensemble(0, 128, 128, ndev=1, batch=256, large=True) as e:
        assert e.batch == 256 and L.lib().perc_ensemble_batch(e.h) == 256
        e.set_batch_large(False)
        assert e.batch == 0 and L.lib().perc_ensemble_batch(e.h) == 0
    with api.Ensemble(0, 129, 128, ndev=1, batch=256, large=True) as e:
        assert e.batch == 0
