"""The batched cluster geometry (perc_batch_clusters_geom, the GEOM
instantiations of k_batch_clusters): every field of the geometry record and
every entry of the octave rows equal to api.cluster_geometry_host (itself held
to brute-force pair sums in test_batch_geometry_host.py) -- integers, no
tolerance -- and the cluster record and histogram bit for bit the plain call's:

* random occupancies, 3 kinds x 2 lattices, from the empty lattice to the full;
* the shapes where the kernel can go wrong: one interior row, the thread-count
  boundaries of scan_threads, the 16384-site caps in both aspects at full
  occupancy (one cluster of every site: the largest sums, 32-bit squares) and
  near the threshold;
* stripes, combs, spirals (tests/label_patterns.py): many spanning clusters;
* seeds against orders, an item's place in the launch, a call split at the
  chunk bound, correlation_curve batched against the host, the errors.

The triangular lattice at an odd m cannot reach the kernel: perc_ctx_create
refuses it (H7); test_odd_m_triangular holds that and the host reference's
positions there."""
import numpy as np
import pytest

import label_patterns as LP
from percolation_amd import _lib as L
from percolation_amd import api

pytestmark = pytest.mark.gpu
KINDS = [L.BOND, L.SITE, L.SITEBOND]
FIELDS = [f for f in L.GEOM_DTYPE.names if f != "pad"]
# (bond, site, mixed: the bonds at 85 % of the sites) thresholds, square / triangular
PC = {0: (0.5, 0.593, 0.65), 1: (0.347, 0.5, 0.45)}


def kw_of(kind, so, bo, ns, nbc):
    kw = {}
    if kind != L.BOND:
        kw.update(site_orders=so, item_nsites=ns)
    if kind != L.SITE:
        kw.update(bond_orders=bo, item_nbonds=nbc)
    return kw


def host(lat, kind, so, ns, bo, nbc):
    return api.cluster_geometry_host(*lat, kind, so if kind != L.BOND else None, int(ns),
                                     bo if kind != L.SITE else None, int(nbc))


def check(geom, rows, want, what):
    assert len(geom) == len(want) and rows.shape == (len(want), 96) and rows.dtype == np.int64
    for i, (rec, row) in enumerate(want):
        for f in FIELDS:
            assert geom[i][f] == rec[f], (what, i, f, geom[i], rec)
        assert geom[i]["pad"] == 0
        assert np.array_equal(rows[i], row), (what, i, rows[i], row)


def counts(lat, kind, fracs):
    """(nsites, nbonds) of the fractions of the kind's threshold (None: the
    empty lattice, inf: every element)"""
    t, nb = lat[1] * lat[2], api.nbonds(*lat)
    pc = PC[lat[0]][KINDS.index(kind)]

    def of(N, p, f):
        return 0 if f is None else N if f == np.inf else min(N, round(f * p * N))

    ns = [of(t, 0.85 if kind == L.SITEBOND else pc, 1.0 if kind == L.SITEBOND and f not in (None, np.inf) else f)
          for f in fracs]
    nbc = [of(nb, pc, f) for f in fracs]
    return (np.array(ns if kind != L.BOND else [0] * len(fracs), np.int32),
            np.array(nbc if kind != L.SITE else [0] * len(fracs), np.int32))


_REF = {}


def reference(lat, kind, fracs=(None, 0.8, 1.0, 1.3, np.inf), seeds=((626504, 58302), (7, 11))):
    """(site orders, bond orders, item_trial, nsites, nbonds, [(record, rows)])
    of a lattice and kind, computed once: the trials of `seeds`, each at every
    fraction of `fracs`"""
    key = (lat, kind, fracs, seeds)
    if key not in _REF:
        t, nb = lat[1] * lat[2], api.nbonds(*lat)
        so = np.stack([api.shuffled_ids(t, s) for s, _ in seeds])
        bo = np.stack([api.shuffled_ids(nb, s) for _, s in seeds])
        ns, nbc = (np.tile(c, len(seeds)) for c in counts(lat, kind, fracs))
        it = np.repeat(np.arange(len(seeds), dtype=np.int32), len(fracs))
        want = [host(lat, kind, so[it[i]], ns[i], bo[it[i]], nbc[i]) for i in range(len(it))]
        for a in (so, bo, it, ns, nbc):
            a.setflags(write=False)
        _REF[key] = (so, bo, it, ns, nbc, want)
    return _REF[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lat", [(0, 20, 17, 0), (1, 16, 24, 0)])
def test_random_occupancies(lat, kind):
    """p = 0, below, at and above the threshold, 1; and the cluster record and
    the histogram are the plain call's, bit for bit"""
    so, bo, it, ns, nbc, want = reference(lat, kind)
    assert api.batch_geometry_supported(*lat, 1024)
    with api.Context(*lat) as ctx:
        for nexact in (0, 1024):
            recs, hist, geom, rows = ctx.batch_clusters(kind, it, **kw_of(kind, so, bo, ns, nbc), nexact=nexact,
                                                        geometry=True)
            check(geom, rows, want, (lat, kind, nexact))
            plain = ctx.batch_clusters(kind, it, **kw_of(kind, so, bo, ns, nbc), nexact=nexact)
            assert len(plain) == 2
            assert recs.tobytes() == plain[0].tobytes() and hist.tobytes() == plain[1].tobytes()
        got = ctx.batch_clusters(kind, it, **kw_of(kind, so, bo, ns, nbc), hist=False, geometry=True,
                                 geometry_rows=False)
        assert got[1] is None and got[3] is None
        assert got[0].tobytes() == plain[0].tobytes() and got[2].tobytes() == geom.tobytes()
    # the cases are what they claim
    empty, full, below, above = want[0], want[4], want[1], want[3]
    assert empty[0] == np.zeros((), L.GEOM_DTYPE) and not empty[1].any()
    t = lat[1] * lat[2]
    assert full[0]["n1"] == full[0]["big_n"] == full[0]["root_n"] == t and full[0]["big_root"] == 1
    assert full[0]["g2"] == full[0]["span_g2"] == full[0]["big_g2"] == full[0]["root_g2"] > 0
    assert below[1][:32].sum() > 3 and above[0]["span_n1"] > 0


# one interior row; t = 4096 | 4160 and 8192 | 8281: scan_threads' steps to 512 and 1024
# threads; the 16384-site caps, square and both thin aspects, on both lattices
SHAPES = [(0, 3, 3, 0), (0, 3, 4, 0), (1, 4, 3, 0), (0, 64, 64, 0), (0, 65, 64, 0), (1, 64, 64, 0), (0, 128, 64, 0),
          (0, 91, 91, 0), (1, 128, 64, 0), (0, 128, 128, 0), (1, 128, 128, 0), (0, 3, 5461, 0), (0, 5461, 3, 0),
          (1, 4, 4096, 0), (1, 5460, 3, 0)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lat", SHAPES)
def test_shapes(lat, kind):
    """near the threshold and at full occupancy (one cluster of every site:
    (sum c)^2 and n_c sum |r|^2 far past 2^31 at the caps)"""
    so, bo, it, ns, nbc, want = reference(lat, kind, fracs=(1.05, np.inf), seeds=((626504, 58302),))
    assert api.batch_geometry_supported(*lat, 1024)
    with api.Context(*lat) as ctx:
        recs, hist, geom, rows = ctx.batch_clusters(kind, it, **kw_of(kind, so, bo, ns, nbc), nexact=1024,
                                                    geometry=True)
        check(geom, rows, want, (lat, kind))
        plain = ctx.batch_clusters(kind, it, **kw_of(kind, so, bo, ns, nbc), nexact=1024)
        assert recs.tobytes() == plain[0].tobytes() and hist.tobytes() == plain[1].tobytes()
    t = lat[1] * lat[2]
    full = want[1][0]
    assert full["big_n"] == t and full["n2"] == t * t
    if t > 16000:
        assert full["g2"] > 2 ** 32
    if lat[0] == 0:  # the full rectangle's closed form
        assert full["g2"] == t * t * (lat[1] ** 2 + lat[2] ** 2 - 2) // 12


def test_odd_m_triangular():
    with pytest.raises(L.PercError, match="even m"):
        api.Context(1, 7, 6, 0)
    x, y, wx, unit = api.site_positions(1, 7, 6)
    assert (wx, unit) == (3, 4) and y.min() == -1 and len(x) == 42


PATTERNS = {"bond": ("hstripes", "vstripes", "combs", "combs_joined", "spiral"),
            "site": ("hstripes", "vstripes", "combs", "serp"),
            "mixed": ("s:vstripes", "s:combs", "b:vstripes", "b:spiral", "s:vstripes*b:vstripes")}


@pytest.mark.parametrize("kind_name,lat", [("bond", (0, 33, 31, 0)), ("site", (0, 128, 128, 0)),
                                           ("mixed", (1, 64, 40, 0))])
def test_structured_occupancies(kind_name, lat):
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
        recs, hist, geom, rows = ctx.batch_clusters(kind, it, **kw_of(kind, so, bo, ns, nbc), nexact=64, geometry=True)
    check(geom, rows, want, (lat, kind_name))
    many = {"bond": "vstripes", "site": "vstripes", "mixed": "s:vstripes*b:vstripes"}[kind_name]
    i = [c[0] for c in cases].index(many)
    assert recs[i]["nspan"] == (lat[1] + 1) // 2  # every cluster spans, every other column
    for a, b in (("span_n1", "n1"), ("span_n2", "n2"), ("span_g2", "g2")):
        assert want[i][0][a] == want[i][0][b] > 0
    assert geom[i]["big_root"] == 1 and geom[i]["big_n"] == lat[2]  # equal columns: the tie goes to the smallest root


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
        a = ctx.batch_clusters(kind, it, **kw_of(kind, so, bo, ns, nbc), nexact=64, geometry=True)
        skw = {k.replace("orders", "seeds"): (seeds_s if k == "site_orders" else seeds_b if k == "bond_orders" else v)
               for k, v in kw_of(kind, so, bo, ns, nbc).items()}
        b = ctx.batch_clusters(kind, it, **skw, nexact=64, geometry=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert a[2]["g2"].max() > 0 and a[3][:, :32].sum() > 10
    check(a[2][1:3], a[3][1:3], [host(lat, kind, so[it[i]], ns[i], bo[it[i]], nbc[i]) for i in (1, 2)], (lat, kind))


@pytest.mark.parametrize("kind", KINDS)
def test_place_independence(kind):
    """one item at the start, in the middle and at the end of a call, between
    items of another trial: identical records and rows"""
    lat = (0, 20, 17, 0)
    so, bo, it, ns, nbc, want = reference(lat, kind)
    n = 301
    sel = np.where(np.arange(n) % 150 == 0, 2, np.arange(n) % len(it))  # item 2 at 0, 150, 300
    with api.Context(*lat) as ctx:
        _, _, geom, rows = ctx.batch_clusters(kind, it[sel], **kw_of(kind, so, bo, ns[sel], nbc[sel]), nexact=64,
                                              geometry=True)
    check(geom, rows, [want[j] for j in sel], (lat, kind))
    for i in (150, 300):
        assert geom[i] == geom[0] and np.array_equal(rows[i], rows[0])


def test_chunk_bound_split():
    """a call past the 64 MB bound on an item's outputs (13508 items at nexact
    = 1024 with the geometry's record and rows) is split: the items of the
    second launch, their trials numbered afresh, give the rows of the first"""
    lat, kind = (0, 10, 10, 0), L.SITEBOND
    so, bo, it, ns, nbc, want = reference(lat, kind)
    n = 14000
    bound = (64 << 20) // (4 * (1024 + 32) + L.GEOM_DTYPE.itemsize + 8 * 96)
    assert bound < n - 100
    sel = (np.arange(n) + np.arange(n) // bound) % len(it)
    with api.Context(*lat) as ctx:
        recs, hist, geom, rows = ctx.batch_clusters(kind, it[sel], **kw_of(kind, so, bo, ns[sel], nbc[sel]),
                                                    nexact=1024, geometry=True)
        first = ctx.batch_clusters(kind, it, **kw_of(kind, so, bo, ns, nbc), nexact=1024)
    wrec = np.array([w[0] for w in want], dtype=L.GEOM_DTYPE)
    wrow = np.stack([w[1] for w in want])
    assert np.array_equal(geom, wrec[sel]) and np.array_equal(rows, wrow[sel])
    assert np.array_equal(recs, first[0][sel]) and np.array_equal(hist, first[1][sel])


@pytest.mark.parametrize("kind", KINDS)
def test_correlation_curve_paths_agree(kind):
    """batch=256 against batch=0 (the host, item by item) and against the
    device shuffle, exactly"""
    grid = [(0.5, 0.9), (0.7, 0.7), (0.9, 0.6), (1.0, 1.0)] if kind == L.SITEBOND else [0.3, 0.5, 0.6, 1.0]
    args = dict(lattice=0, m=20, n=20, pbc=0, kind=kind, grid=grid, master=58302, numtrials=3, nexact=32)
    h = api.correlation_curve(batch=0, **args)
    with api.Context(0, 20, 20, 0) as ctx:
        b = api.correlation_curve(batch=256, ctx=ctx, **args)
        d = api.correlation_curve(batch=8, device_shuffle=True, ctx=ctx, **args)
    for o in (b, d):
        assert o["trials"] == h["trials"]
        for k in ("stats", "hist", "sums", "rows"):
            assert np.array_equal(o[k], h[k]), k
        for k in ("xi", "big_r2", "rs2"):
            assert np.array_equal(o[k], h[k], equal_nan=True), k
    assert h["sums"][:, 0].tolist() == [3] * 4 and h["sums"][-1, 1] == 3 * 400
    assert np.isfinite(h["xi"][:3]).all() and (h["xi"][:3] > 0).all()


def test_errors_and_context_state():
    """pbc = 1 and a bad kind: PERC_EINVAL / ValueError before any device
    call; the context's single-realisation state is untouched by the calls"""
    assert not api.batch_geometry_supported(0, 10, 10, 1, 0) and api.batch_clusters_supported(0, 10, 10, 1, 0)
    with api.Context(0, 10, 10, 1) as ctx:
        bo = api.shuffled_ids(ctx.nb, 2)
        with pytest.raises(L.PercError, match="PERC_EINVAL.*perc_batch_geometry_supported"):
            ctx.batch_clusters(L.BOND, [0], bond_orders=bo, item_nbonds=[5], geometry=True)
        assert L.lib().perc_last_error().decode().startswith("perc_batch_clusters_geom:")
        with pytest.raises(L.PercError, match="PERC_EINVAL.*perc_batch_geometry_supported"):
            ctx.batch_clusters(L.BOND, [0], bond_seeds=[3], item_nbonds=[5], geometry=True)
        assert L.lib().perc_last_error().decode().startswith("perc_batch_clusters_geom_seeded:")
        ctx.batch_clusters(L.BOND, [0], bond_orders=bo, item_nbonds=[5])  # (the plain call takes pbc)
        with pytest.raises(ValueError, match="pbc"):
            api.correlation_curve(kind=L.BOND, grid=[0.5], ctx=ctx)
    lat = (0, 50, 50, 0)
    with api.Context(*lat) as ctx:
        t, nb = ctx.t, ctx.nb
        s1, b1 = api.shuffled_ids(t, 1), api.shuffled_ids(nb, 2)
        both = dict(site_orders=s1, bond_orders=b1)
        for kw in (dict(kind=L.BONDSITE, **both, item_nsites=[5], item_nbonds=[5]),
                   dict(kind=7, **both, item_nsites=[5], item_nbonds=[5]),
                   dict(kind=L.SITEBOND, **both, item_nsites=[5], item_nbonds=[5], nexact=1025),
                   dict(kind=L.BOND, site_orders=s1, item_nbonds=[5]),
                   dict(kind=L.SITE, site_orders=s1, item_nsites=[t + 2]),
                   dict(kind=L.BOND, bond_orders=b1, item_nbonds=[5], item_trial=[1])):
            kw.setdefault("item_trial", [0])
            with pytest.raises(L.PercError, match="PERC_EINVAL"):
                ctx.batch_clusters(geometry=True, **kw)
            assert L.lib().perc_last_error().decode().startswith("perc_batch_clusters_geom")
        with pytest.raises(ValueError, match="kind"):
            api.correlation_curve(kind=L.BONDSITE, grid=[0.5], ctx=ctx)
        lib = L.lib()
        one, five = np.zeros(1, np.int32), np.full(1, 5, np.int32)
        out, geom = np.zeros(1, dtype=L.CLUSTER_DTYPE), np.zeros(1, dtype=L.GEOM_DTYPE)
        raw = lambda nitems, g: lib.perc_batch_clusters_geom(  # noqa: E731
            ctx.h, L.BOND, 1, None, L.ptr(b1), nitems, L.ptr(one), None, L.ptr(five), 0, L.ptr(out), None, g, None)
        assert raw(1, None) == -1 and raw(0, None) == 0 and raw(1, L.ptr(geom)) == 0 and geom["n1"][0] > 0
        # the single-realisation state
        order = api.shuffled_ids(nb, 626504)
        ctx.occupy(L.BOND, bond_order=order, nbonds_=2940)
        li = ctx.label(canon=True)
        nums = ctx.label_numbers(L.BOND)
        sizes, occ = ctx.cluster_sizes(), ctx.occupancy()
        ctx.batch_clusters(L.SITE, [0, 0], site_orders=s1, item_nsites=[1500, 2500], geometry=True)
        ctx.batch_clusters(L.BOND, [0, 1], bond_seeds=[3, 4], item_nbonds=[2000, 2600], geometry=True)
        assert ctx.cluster_sizes() == sizes
        after = ctx.label_numbers(L.BOND)
        assert np.array_equal(after["bond_label"], nums["bond_label"]) and after["perccln"] == nums["perccln"]
        assert all(np.array_equal(x, y) for x, y in zip(ctx.occupancy(), occ))
        again = ctx.label(canon=True)
        assert np.array_equal(again["canon"], li["canon"]) and again["nclusters"] == li["nclusters"]
