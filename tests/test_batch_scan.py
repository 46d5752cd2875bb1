"""The batched threshold scans (perc_batch_scan, k_batch_scan): one workgroup
bisects each small-lattice trial, checked trial by trial against the single
path (perc_first_spanning / perc_first_spanning_mixed + perc_cluster_sizes),
the reference's bond_perc / site_perc / sb_perc text files and the host
replay of bs_perc's intended rule:

* every trial of 8 lattices x {bond, site}, the 128 x 128 cap on both
  lattices;
* the goldens through api.threshold_scan / api.mixed_scan(batch=16) and the
  Fortran drivers' `batch` key, byte for byte;
* nothing spans, the shuffle's spill slot inside the scanned prefix, one
  order at both ends of a 200-trial call, ntrials 0 and 1, the context's
  single-realisation state left alone, the argument errors.

The single path's result of a (lattice, kind) is computed once and shared."""
import numpy as np
import pytest

import golden_io as G
import test_fortran_drivers as F
from percolation_amd import _lib as L
from percolation_amd import api

pytestmark = pytest.mark.gpu
LATTICES = [(0, 10, 10, 0), (0, 10, 10, 1), (1, 10, 10, 0), (1, 12, 9, 1), (0, 5, 3, 0), (0, 37, 23, 0),
            (0, 50, 50, 0), (1, 50, 50, 0)]
CAP = [(0, 128, 128, 0), (1, 128, 128, 0)]
KINDS = [L.BOND, L.SITE]
PERC = [v for v in G.variants() if G.meta(v)["kind"] in ("bond_perc", "site_perc")]
SB = [v for v in G.variants() if G.meta(v)["kind"] == "sb_perc"]


def orders_kw(kind, orders):
    return {"bond_orders" if kind == L.BOND else "site_orders": orders}


def single(ctx, order, kind):
    """the single path: first spanning count, then the sizes on the context
    that call leaves behind"""
    first = api.first_spanning(ctx, order, kind)
    maxcs, span = ctx.cluster_sizes()
    return dict(first=first, maxcs=maxcs, span_size=span)


_REF = {}


def reference(lat, kind, ntrials):
    key = (lat, kind, ntrials)
    if key not in _REF:
        seeds = api.trial_seeds(58302, 8, scale=1000000)[:ntrials]
        with api.Context(*lat) as ctx:
            N = ctx.nb if kind == L.BOND else ctx.t
            orders = np.stack([api.shuffled_ids(N, int(s)) for s in seeds])
            want = [single(ctx, o, kind) for o in orders]
        _REF[key] = (orders, want)
    return _REF[key]


def check_items(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for k in ("first", "maxcs", "span_size"):
            assert g[k] == w[k], (what, i, k, g, w)
        assert g["nspan"] == (1 if g["first"] > 0 else 0), (what, i, g)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lat", LATTICES)
def test_single_path_parity(lat, kind):
    orders, want = reference(lat, kind, 8)
    with api.Context(*lat) as ctx:
        got = ctx.batch_scan(kind, **orders_kw(kind, orders))
    check_items(got, want, (lat, kind))
    print("lattice %s kind %d: first %s" % (lat, kind, [g["first"] for g in got]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lat", CAP)
def test_size_cap(lat, kind):
    assert api.scan_supported(*lat)
    orders, want = reference(lat, kind, 2)
    with api.Context(*lat) as ctx:
        got = ctx.batch_scan(kind, **orders_kw(kind, orders))
    check_items(got, want, (lat, kind))
    assert all(g["first"] > 0 for g in got)


@pytest.mark.parametrize("v", PERC)
def test_threshold_scan_goldens(v):
    md = G.meta(v)
    p = md["params"]
    kind = L.BOND if md["kind"] == "bond_perc" else L.SITE
    rows = api.threshold_scan(p["lattice"], p["m"], p["n"], p["pbc"], kind, p["seed"], p["numtrials"],
                              batch=16)
    assert api.fmt_perc_rows(rows).encode() == G.text(v, md["kind"] + ".txt")


@pytest.mark.parametrize("v", SB)
def test_sb_perc_goldens(v):
    p = G.meta(v)["params"]
    rows = api.mixed_scan(p["lattice"], p["m"], p["n"], p["pbc"], L.BOND, p["seed"], p["points"],
                          p["iters"], batch=16)
    assert api.fmt_mixed_rows(rows).encode() == G.text(v, "sb_perc.txt")


def test_bs_intended_rule_equals_replay():
    lat, m, n, pbc = 1, 20, 16, 1
    t, nb = m * n, api.nbonds(lat, m, n, pbc)
    tb = int(0.6 * nb)
    so = np.stack([api.shuffled_ids(t, seed) for seed in range(1, 12)])
    bo = np.stack([api.shuffled_ids(nb, seed + 77) for seed in range(1, 12)])
    with api.Context(lat, m, n, pbc) as ctx:
        got = ctx.batch_scan(L.SITEBOND, site_orders=so, bond_orders=bo, scan=L.SITE, fixed=tb)
        for i, g in enumerate(got):
            assert g["first"] == api.bs_perc_replay(lat, m, n, pbc, so[i], t, bo[i], tb, False), i
            assert g["maxcs"] == 0 and g["span_size"] == 0
        kw = dict(scan=L.SITE, master=229102, points=[0.5, 0.6], iters=10, as_built=False, ctx=ctx)
        on = api.mixed_scan(lat, m, n, pbc, batch=8, **kw)
        off = api.mixed_scan(lat, m, n, pbc, batch=0, **kw)
    assert on == off and len(on) == 20
    assert any(r["first"] > 0 for r in on)


def test_nothing_spans():
    m = n = 8
    order = api.shuffled_ids(m * n, 4711)
    order[(order > 3 * m) & (order <= 4 * m)] = 0  # lattice row 3 never occupied
    with api.Context(0, m, n, 0) as ctx:
        got = ctx.batch_scan(L.SITE, site_orders=order)[0]
        want = single(ctx, order, L.SITE)  # (left at the full count)
        assert want["first"] == 0
        assert got["first"] == 0 and got["span_size"] == 0 and got["nspan"] == 0
        assert got["maxcs"] == want["maxcs"] > 0
        # no site occupied: no bond can connect
        so, bo = api.shuffled_ids(m * n, 5), api.shuffled_ids(ctx.nb, 6)
        g = ctx.batch_scan(L.SITEBOND, site_orders=so, bond_orders=bo, scan=L.BOND, fixed=0)[0]
        assert g["first"] == 0 and g["nspan"] == 0
        assert api.first_spanning_mixed(ctx, L.BOND, so, 0, bo, ctx.nb) == 0


def column_bonds(m, n, col):
    b1, b2 = api.bond_list(0, m, n, 0)
    return [k + 1 for k in range(len(b1)) if b2[k] - b1[k] == m and (b1[k] - 1) % m == col]


def test_spill_slot():
    """the shuffle's spill entry 0 inside the scanned prefix takes a position
    and is no bond: the column completes with the entry just after it"""
    m = n = 8
    nb = api.nbonds(0, m, n, 0)
    col = column_bonds(m, n, 3)
    assert len(col) == 7
    ids = col[:6] + [0] + col[6:] + [k for k in range(1, nb + 1) if k not in col]
    order = np.array(ids, np.int32)
    assert len(order) == nb + 1 and order[6] == 0
    with api.Context(0, m, n, 0) as ctx:
        got = ctx.batch_scan(L.BOND, bond_orders=order)[0]
        want = single(ctx, order, L.BOND)
    assert want["first"] == 8
    check_items([got], [want], "spill")
    assert got["span_size"] == 7


def test_batch_mechanics():
    lat = (0, 10, 10, 0)
    with api.Context(*lat) as ctx:
        nb = ctx.nb
        orders = np.stack([api.shuffled_ids(nb, 1000 + i) for i in range(200)])
        orders[199] = orders[0]
        want = [single(ctx, o, L.BOND) for o in orders]
        # a previously occupied context keeps its state over a batch call
        ctx.occupy(L.BOND, bond_order=orders[5], nbonds_=int(0.6 * nb))
        before = ctx.label()
        got = ctx.batch_scan(L.BOND, bond_orders=orders)
        assert ctx.label() == before
        check_items(got, want, "200 trials")
        assert got[0] == got[199]
        assert ctx.batch_scan(L.BOND, bond_orders=orders[:0]) == []
        assert ctx.batch_scan(L.BOND, bond_orders=orders[:1]) == got[:1]
        assert ctx.batch_scan(L.BOND, bond_orders=orders[7]) == got[7:8]


def test_errors_are_einval():
    with api.Context(0, 129, 128, 0) as ctx:
        assert not api.scan_supported(0, 129, 128, 0)
        with pytest.raises(L.PercError, match="PERC_EINVAL"):
            ctx.batch_scan(L.BOND, bond_orders=api.shuffled_ids(ctx.nb, 1))
    with api.Context(0, 10, 10, 0) as ctx:
        so, bo = api.shuffled_ids(ctx.t, 1), api.shuffled_ids(ctx.nb, 2)
        for kw in (dict(kind=L.BONDSITE, site_orders=so, bond_orders=bo, fixed=5),
                   dict(kind=L.SITEBOND, site_orders=so, bond_orders=bo),
                   dict(kind=L.SITEBOND, site_orders=so, bond_orders=bo, scan=L.BOND, fixed=ctx.t + 1),
                   dict(kind=L.SITEBOND, site_orders=so, bond_orders=bo, scan=L.SITE, fixed=ctx.nb + 1),
                   dict(kind=L.SITEBOND, site_orders=so, bond_orders=bo, scan=L.SITE, fixed=-1),
                   dict(kind=L.SITEBOND, site_orders=so, bond_orders=bo, scan=3, fixed=5),
                   dict(kind=L.BOND, site_orders=so),
                   dict(kind=L.SITE, bond_orders=bo),
                   dict(kind=L.SITEBOND, site_orders=so, fixed=5)):
            with pytest.raises(L.PercError, match="PERC_EINVAL"):
                ctx.batch_scan(**kw)
        rc = L.lib().perc_batch_scan(ctx.h, L.BOND, L.BOND, -1, None, L.ptr(bo), None, None)
        assert rc == -1


@pytest.mark.parametrize("v", ["sq_bond_perc", "tri_site_perc", "sq_sb_perc"])
def test_fortran_batch_key(v, tmp_path):
    """the drivers with batch=16 in their namelist write the reference's text
    files byte for byte (skips only when the drivers are not built)"""
    md, r = F.run_variant(v, tmp_path, extra=("batch=16",))
    name = md["kind"] + ".txt"
    assert (tmp_path / name).read_bytes() == G.text(v, name)
    assert len(r.stdout.splitlines()) == len(G.text(v, name).splitlines())
