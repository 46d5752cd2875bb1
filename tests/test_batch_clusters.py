"""The batched cluster tables (perc_batch_clusters, k_batch_clusters): one
workgroup per (trial, nsites, nbonds) item, every record field and every
histogram entry held to api.cluster_stats_host (itself checked against scipy
in test_batch_clusters_host.py) exactly -- the results are integers:

* 10 x 10 .. 128 x 128 at every workgroup size, all three kinds, from the
  empty lattice to the whole order, nexact 0, 64 and 1024, hist = NULL;
* stripes, combs and spirals (tests/label_patterns.py): many spanning
  clusters at once, long union chains;
* one item at several places of a call and across the call's chunk bound,
  seeds against orders, cluster_curve batched against the host, the
  context's single-realisation state, the argument errors.

The host reference of an item is computed once, at nexact = 1024; the rows of
a smaller nexact are slices of it."""
import ctypes as C

import numpy as np
import pytest

import label_patterns as LP
from percolation_amd import _lib as L
from percolation_amd import api

pytestmark = pytest.mark.gpu
KINDS = [L.BOND, L.SITE, L.SITEBOND]
# threads beyond the sites; odd m; 256 threads, 10 sites per thread; the first
# 512-thread size; 1024 threads, 16 sites per thread; the largest arena
CASES = ([((0, 10, 10, 0), k) for k in KINDS] + [((0, 33, 31, 0), k) for k in KINDS]
         + [((0, 50, 50, 0), k) for k in KINDS] + [((0, 65, 65, 0), k) for k in KINDS]
         + [((0, 128, 128, 0), k) for k in KINDS] + [((1, 128, 128, 1), L.SITEBOND)])
FIELDS = L.CLUSTER_DTYPE.names
NMAX = 1024


def kw_of(kind, so, bo, ns, nbc):
    kw = {}
    if kind != L.BOND:
        kw.update(site_orders=so, item_nsites=ns)
    if kind != L.SITE:
        kw.update(bond_orders=bo, item_nbonds=nbc)
    return kw


def host(lat, kind, so, ns, bo, nbc):
    return api.cluster_stats_host(*lat, kind, so if kind != L.BOND else None, int(ns),
                                  bo if kind != L.SITE else None, int(nbc), NMAX)


def row_of(row, nexact):
    """the histogram row at a smaller nexact from the one at NMAX"""
    return np.concatenate([row[:nexact], row[NMAX:]])


def check(recs, hist, want, nexact, what):
    assert len(recs) == len(want)
    for i, (rec, row) in enumerate(want):
        for f in FIELDS:
            assert recs[i][f] == rec[f], (what, i, f, recs[i], rec)
        if hist is not None:
            assert np.array_equal(hist[i], row_of(row, nexact)), (what, i)


_REF = {}


def reference(lat, kind):
    """(site orders, bond orders, item_trial, nsites, nbonds, [(record, row)])
    of a lattice and kind: two trials; empty, one element, below / at / above
    the threshold, full, the whole order (and, mixed: lone bonds only, half
    the sites under every bond)"""
    key = (lat, kind)
    if key in _REF:
        return _REF[key]
    t, nb = lat[1] * lat[2], api.nbonds(*lat)
    so = np.stack([api.shuffled_ids(t, s) for s in (626504, 7)])
    bo = np.stack([api.shuffled_ids(nb, s) for s in (58302, 11)])
    tri = lat[0] == 1
    if kind == L.BOND:
        pc = 0.347 if tri else 0.5
        fs, fb = [0] * 7, [0, 1 / nb, 0.8 * pc, pc, 1.2 * pc, 1.0, 1.0 + 1 / nb]
    elif kind == L.SITE:
        pc = 0.5 if tri else 0.593
        fs, fb = [0, 1 / t, 0.8 * pc, pc, 1.2 * pc, 1.0, 1.0 + 1 / t], [0] * 7
    else:
        pc = 0.45 if tri else 0.65  # (bonds, at 85 % of the sites)
        fs = [0, 1 / t, 0.85, 0.85, 0.85, 1.0, 1.0 + 1 / t, 0, 0.5]
        fb = [0, 1 / nb, 0.8 * pc, pc, 1.2 * pc, 1.0, 1.0 + 1 / nb, 0.5, 1.0 + 1 / nb]
    ns = np.array([round(f * t) for f in fs], np.int32)
    nbc = np.array([round(f * nb) for f in fb], np.int32)
    it = (np.arange(len(ns)) % 2).astype(np.int32)
    want = [host(lat, kind, so[it[i]], ns[i], bo[it[i]], nbc[i]) for i in range(len(ns))]
    for a in (so, bo, it, ns, nbc):
        a.setflags(write=False)
    _REF[key] = (so, bo, it, ns, nbc, want)
    return _REF[key]


@pytest.mark.parametrize("lat,kind", CASES)
def test_exact_match(lat, kind):
    so, bo, it, ns, nbc, want = reference(lat, kind)
    assert api.batch_clusters_supported(*lat, NMAX)
    with api.Context(*lat) as ctx:
        for nexact in (0, 64, NMAX):
            recs, hist = ctx.batch_clusters(kind, it, **kw_of(kind, so, bo, ns, nbc), nexact=nexact)
            assert hist.shape == (len(it), nexact + 32)
            check(recs, hist, want, nexact, (lat, kind, nexact))
        recs, hist = ctx.batch_clusters(kind, it, **kw_of(kind, so, bo, ns, nbc), nexact=64, hist=False)
        assert hist is None
        check(recs, None, want, 64, (lat, kind, "no hist"))
    # the cases are what they claim: nothing at 0, one cluster on the full lattice, it spans
    assert want[0][0]["nclusters"] == 0 and want[0][0]["maxcs"] == 0
    assert want[5][0]["nclusters"] == 1 and want[5][0]["nspan"] == 1 and want[5][0]["span_root"] == 1
    assert [f for f in FIELDS if want[5][0][f] != want[6][0][f]] == []
    assert want[2][0]["nspan"] == 0 or lat[1] <= 10
    assert want[4][0]["nspan"] >= 1 or lat[1] <= 10
    if kind == L.SITEBOND:
        lone = np.count_nonzero(bo[it[7]][:nbc[7]])  # (the spill slot is no bond)
        assert want[7][0]["nlone"] == want[7][0]["nclusters"] == lone and want[7][0]["maxcs"] == 1


PATTERNS = {"bond": ("hstripes", "vstripes", "combs", "combs_joined", "spiral"),
            "site": ("hstripes", "vstripes", "combs", "serp"),
            "mixed": ("s:vstripes", "s:combs", "b:vstripes", "b:spiral", "s:vstripes*b:vstripes")}


@pytest.mark.parametrize("kind_name", LP.KINDS)
@pytest.mark.parametrize("lat", [(0, 33, 31, 0), (0, 128, 128, 0), (1, 64, 40, 1)])
def test_structured_occupancies(lat, kind_name):
    """the pattern's elements first in the order, the count its length: up to
    m / 2 spanning clusters at once (span_s1 / span_s2 over all of them) and
    chains as long as the lattice"""
    kind = KINDS[LP.KINDS.index(kind_name)]
    t, nb = lat[1] * lat[2], api.nbonds(*lat)
    cases = [c for c in LP.cases(kind_name, *lat) if c[0] in PATTERNS[kind_name]]
    assert len(cases) == len(PATTERNS[kind_name])
    so = np.stack([LP.order_row(LP.ordered(s, "perm", 3), t) if s is not None else LP.order_row([], t)
                   for _, s, _ in cases])
    bo = np.stack([LP.order_row(LP.ordered(b, "perm", 4), nb) if b is not None else LP.order_row([], nb)
                   for _, _, b in cases])
    ns = np.array([len(s) if s is not None else 0 for _, s, _ in cases], np.int32)
    nbc = np.array([len(b) if b is not None else 0 for _, _, b in cases], np.int32)
    it = np.arange(len(cases), dtype=np.int32)
    want = [host(lat, kind, so[i], ns[i], bo[i], nbc[i]) for i in it]
    with api.Context(*lat) as ctx:
        recs, hist = ctx.batch_clusters(kind, it, **kw_of(kind, so, bo, ns, nbc), nexact=NMAX)
    check(recs, hist, want, NMAX, (lat, kind_name))
    nspan = {c[0]: int(w[0]["nspan"]) for c, w in zip(cases, want)}
    print("lattice %s %s: nspan %s" % (lat, kind_name, nspan))
    many = {"bond": "vstripes", "site": "vstripes", "mixed": "s:vstripes*b:vstripes"}[kind_name]
    assert nspan[many] == (lat[1] + 1) // 2
    i = [c[0] for c in cases].index(many)
    assert want[i][0]["span_s1"] == want[i][0]["s1"] and want[i][0]["span_s2"] == want[i][0]["s2"]


@pytest.mark.parametrize("kind", KINDS)
def test_place_independence(kind):
    """one item at the start, in the middle and at the end of a call, between
    items of another trial: identical rows"""
    lat = (0, 50, 50, 0)
    so, bo, it, ns, nbc, want = reference(lat, kind)
    n = 301
    sel = np.where(np.arange(n) % 150 == 0, 3, np.arange(n) % len(it))  # item 3 at 0, 150, 300
    with api.Context(*lat) as ctx:
        recs, hist = ctx.batch_clusters(kind, it[sel], **kw_of(kind, so, bo, ns[sel], nbc[sel]), nexact=64)
    check(recs, hist, [want[j] for j in sel], 64, (lat, kind))
    for i in (150, 300):
        assert recs[i] == recs[0] and np.array_equal(hist[i], hist[0])


def test_chunk_bound_split():
    """a call past the 64 MB bound on the histogram rows (15887 items at
    nexact = 1024) is split: the items of the second launch, their trials
    numbered afresh, give the rows of the first"""
    lat, kind = (0, 10, 10, 0), L.SITEBOND
    so, bo, it, ns, nbc, want = reference(lat, kind)
    n = 16000
    assert (64 << 20) // (4 * (NMAX + 32)) < n - 100
    sel = (np.arange(n) + np.arange(n) // 15887) % len(it)
    with api.Context(*lat) as ctx:
        recs, hist = ctx.batch_clusters(kind, it[sel], **kw_of(kind, so, bo, ns[sel], nbc[sel]), nexact=NMAX)
    wrec = np.array([want[j][0] for j in range(len(it))], dtype=L.CLUSTER_DTYPE)
    wrow = np.stack([want[j][1] for j in range(len(it))])
    assert np.array_equal(recs, wrec[sel])
    assert np.array_equal(hist, wrow[sel])


@pytest.mark.parametrize("kind", KINDS)
def test_seeded_equals_orders(kind):
    lat = (0, 50, 50, 0)
    seeds_s = np.array([626504, 7, 12345, 1, 99, 8811064], np.int32)
    seeds_b = seeds_s[::-1].copy()
    with api.Context(*lat) as ctx:
        so = np.stack([api.shuffled_ids(ctx.t, int(s)) for s in seeds_s])
        bo = np.stack([api.shuffled_ids(ctx.nb, int(s)) for s in seeds_b])
        it = np.array([5, 0, 3, 3, 1, 4, 2, 5], np.int32)
        ns = np.array([0, 1500, 1482, 2501, 2500, 1600, 900, 1700], np.int32)
        nbc = np.array([4901, 2450, 2400, 0, 4900, 2600, 3000, 1], np.int32)
        a = ctx.batch_clusters(kind, it, **kw_of(kind, so, bo, ns, nbc), nexact=64)
        skw = {k.replace("orders", "seeds"): (seeds_s if k == "site_orders" else seeds_b if k == "bond_orders" else v)
               for k, v in kw_of(kind, so, bo, ns, nbc).items()}
        b = ctx.batch_clusters(kind, it, **skw, nexact=64)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[0]["nclusters"].max() > 10


@pytest.mark.parametrize("kind", KINDS)
def test_cluster_curve_paths_agree(kind):
    """batch=256 against batch=0 (the host, item by item) and against the
    device shuffle, exactly"""
    grid = [(0.5, 0.9), (0.7, 0.7), (0.9, 0.6), (1.0, 1.0)] if kind == L.SITEBOND else [0.3, 0.5, 0.6, 1.0]
    args = dict(lattice=0, m=20, n=20, pbc=0, kind=kind, grid=grid, master=58302, numtrials=3, nexact=32)
    th, sh, hh = api.cluster_curve(batch=0, **args)
    with api.Context(0, 20, 20, 0) as ctx:
        tb, sb, hb = api.cluster_curve(batch=256, ctx=ctx, **args)
        td, sd, hd = api.cluster_curve(batch=8, device_shuffle=True, ctx=ctx, **args)
    assert th == tb == td
    assert np.array_equal(sh, sb) and np.array_equal(sh, sd)
    assert np.array_equal(hh, hb) and np.array_equal(hh, hd)
    assert sh[:, 0].tolist() == [3] * 4 and sh[-1, 2] == 3


def test_context_state_untouched():
    lat = (0, 50, 50, 0)
    so, bo, it, ns, nbc, want = reference(lat, L.SITEBOND)
    with api.Context(*lat) as ctx:
        order = api.shuffled_ids(ctx.nb, 626504)
        ctx.occupy(L.BOND, bond_order=order, nbonds_=2940)
        li = ctx.label(canon=True)
        nums = ctx.label_numbers(L.BOND)
        sizes = ctx.cluster_sizes()
        occ = ctx.occupancy()
        ctx.batch_clusters(L.SITEBOND, it, **kw_of(L.SITEBOND, so, bo, ns, nbc), nexact=64)
        ctx.batch_clusters(L.BOND, it, bond_seeds=[3, 4], item_nbonds=nbc, nexact=0)
        assert ctx.cluster_sizes() == sizes
        after = ctx.label_numbers(L.BOND)
        assert np.array_equal(after["bond_label"], nums["bond_label"]) and after["perccln"] == nums["perccln"]
        assert np.array_equal(after["csize"], nums["csize"])
        assert all(np.array_equal(x, y) for x, y in zip(ctx.occupancy(), occ))
        again = ctx.label(canon=True)
        assert np.array_equal(again["canon"], li["canon"]) and again["nclusters"] == li["nclusters"]


def test_errors_are_einval():
    with api.Context(0, 129, 128, 0) as ctx:
        assert not api.batch_clusters_supported(0, 129, 128, 0, 0)
        with pytest.raises(L.PercError, match="PERC_EINVAL.*perc_batch_clusters_supported"):
            ctx.batch_clusters(L.BOND, [0], bond_orders=api.shuffled_ids(ctx.nb, 1), item_nbonds=[5])
    with api.Context(0, 10, 10, 0) as ctx:
        t, nb = ctx.t, ctx.nb
        so, bo = api.shuffled_ids(t, 1), api.shuffled_ids(nb, 2)
        both = dict(site_orders=so, bond_orders=bo)
        for kw in (dict(kind=L.BONDSITE, **both, item_nsites=[5], item_nbonds=[5]),
                   dict(kind=L.SITEBOND, **both, item_nsites=[5], item_nbonds=[5], nexact=-1),
                   dict(kind=L.SITEBOND, **both, item_nsites=[5], item_nbonds=[5], nexact=1025),
                   dict(kind=L.BOND, site_orders=so, item_nbonds=[5]),      # the order list the kind reads
                   dict(kind=L.SITE, bond_orders=bo, item_nsites=[5]),
                   dict(kind=L.SITEBOND, site_orders=so, item_nsites=[5], item_nbonds=[5]),
                   dict(kind=L.BOND, bond_orders=bo),                       # the count list the kind reads
                   dict(kind=L.SITE, site_orders=so, item_nbonds=[5]),
                   dict(kind=L.SITEBOND, **both, item_nsites=[5]),
                   dict(kind=L.BOND, bond_orders=bo, item_nbonds=[5], item_trial=[1]),
                   dict(kind=L.BOND, bond_orders=bo, item_nbonds=[5], item_trial=[-1]),
                   dict(kind=L.BOND, bond_orders=bo, item_nbonds=[-1]),
                   dict(kind=L.BOND, bond_orders=bo, item_nbonds=[nb + 2]),
                   dict(kind=L.SITE, site_orders=so, item_nsites=[-1]),
                   dict(kind=L.SITE, site_orders=so, item_nsites=[t + 2]),
                   dict(kind=L.SITEBOND, **both, item_nsites=[t + 2], item_nbonds=[5]),
                   dict(kind=L.SITEBOND, **both, item_nsites=[5], item_nbonds=[nb + 2]),
                   dict(kind=L.SITEBOND, site_seeds=[1], item_nsites=[5], item_nbonds=[5]),  # seeded: a seed list
                   dict(kind=L.BOND, site_seeds=[1], item_nbonds=[5])):
            kw.setdefault("item_trial", [0])
            with pytest.raises(L.PercError, match="PERC_EINVAL"):
                ctx.batch_clusters(**kw)
            assert L.lib().perc_last_error().decode().startswith("perc_batch_clusters")
        lib = L.lib()
        one = np.zeros(1, np.int32)
        out = np.zeros(1, dtype=L.CLUSTER_DTYPE)
        five = np.full(1, 5, np.int32)
        raw = lambda ntrials, nitems, o: lib.perc_batch_clusters(  # noqa: E731
            ctx.h, L.BOND, ntrials, None, L.ptr(bo), nitems, L.ptr(one), None, L.ptr(five), 0, o, None)
        assert raw(-1, 1, L.ptr(out)) == -1 and raw(1, -1, L.ptr(out)) == -1 and raw(1, 1, None) == -1
        assert lib.perc_batch_clusters(None, L.BOND, 1, None, L.ptr(bo), 1, L.ptr(one), None, L.ptr(five), 0,
                                       L.ptr(out), None) == -1
        # nitems == 0 is PERC_OK, with or without lists; the whole-order counts are accepted
        assert raw(1, 0, None) == 0 and raw(0, 0, None) == 0
        recs, hist = ctx.batch_clusters(L.SITEBOND, [0], **both, item_nsites=[t + 1], item_nbonds=[nb + 1])
        assert recs[0]["nclusters"] == 1 and recs[0]["s1"] == t + nb and hist.shape == (1, 32)
        assert C.sizeof(L.ClusterItem) == out.itemsize
