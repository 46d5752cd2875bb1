"""The clusters' geometry on the host: api.cluster_geometry_host (the
reference every GPU test of Context.batch_clusters(geometry=True) compares
with) against a brute-force pairwise sum over scipy's connected components,
the embedding (every bond has d2 = unit), the closed form of a full rectangle,
the record's invariants, the host-only predicate and correlation_curve(batch=0).
No device; everything is an integer and compared exactly."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from percolation_amd import _lib as L
from percolation_amd import api

GEOMS = [(0, 7, 5, 0), (0, 12, 12, 0), (0, 3, 11, 0), (1, 8, 6, 0), (1, 12, 11, 0), (1, 7, 6, 0)]
KINDS = [L.BOND, L.SITE, L.SITEBOND]
FIELDS = [f for f in L.GEOM_DTYPE.names if f != "pad"]


def d2(lat, m, i, j):
    """the definition, site by site (0-based site numbers)"""
    ri, ci, rj, cj = i // m, i % m, j // m, j % m
    if lat == L.SQUARE:
        return (ci - cj) ** 2 + (ri - rj) ** 2
    yi, yj = 2 * ri - (ci & 1), 2 * rj - (cj & 1)
    return 3 * (ci - cj) ** 2 + (yi - yj) ** 2


def brute(lat, m, n, kind, so, ns, bo, nbc):
    """the record and rows from scipy's components and the O(n^2) pair sums,
    in Python integers"""
    b1, b2 = api.bond_list(lat, m, n, 0)
    t, nb = m * n, len(b1)
    socc, bocc = np.ones(t + 1, dtype=bool), np.ones(nb, dtype=bool)
    if kind != L.BOND:
        socc[:] = False
        ids = np.asarray(so[:ns])
        socc[ids[ids > 0]] = True
    if kind != L.SITE:
        bocc[:] = False
        ids = np.asarray(bo[:nbc])
        bocc[ids[ids > 0] - 1] = True
    e = bocc & socc[b1] & socc[b2]
    g = sp.coo_matrix((np.ones(int(e.sum()), np.int8), (b1[e], b2[e])), shape=(t + 1, t + 1))
    _, comp = connected_components(g, directed=False)
    if kind == L.BOND:
        member = np.zeros(t + 1, dtype=bool)
        member[b1[e]] = True
        member[b2[e]] = True
    else:
        member = socc.copy()
    member[0] = False
    rec = dict.fromkeys(FIELDS, 0)
    rows = [0] * 96
    best = root = None
    for c in np.unique(comp[member]):
        sites = [int(s) for s in np.nonzero(member & (comp == c))[0]]
        nc = len(sites)
        G = sum(d2(lat, m, sites[a] - 1, sites[b] - 1) for a in range(nc) for b in range(a + 1, nc))
        spans = sites[0] <= m and sites[-1] > t - m
        rec["n1"] += nc
        rec["n2"] += nc * nc
        rec["g2"] += G
        b = nc.bit_length() - 1
        rows[b] += 1
        rows[32 + b] += nc * nc
        rows[64 + b] += G
        if spans:
            rec["span_n1"] += nc
            rec["span_n2"] += nc * nc
            rec["span_g2"] += G
            if root is None or sites[0] < root:
                root, rec["root_n"], rec["root_g2"] = sites[0], nc, G
        if best is None or (nc, -sites[0]) > best:
            best = (nc, -sites[0])
            rec["big_root"], rec["big_n"], rec["big_g2"] = sites[0], nc, G
    return rec, rows


def cases(lat, m, n, kind):
    t, nb = m * n, api.nbonds(lat, m, n, 0)
    so, bo = api.shuffled_ids(t, 4711), api.shuffled_ids(nb, 4712)
    fr = [0.0, 0.25, 0.45, 0.6, 0.8, 1.0]
    if kind == L.BOND:
        return [(None, 0, bo, round(f * nb)) for f in fr]
    if kind == L.SITE:
        return [(so, round(f * t), None, 0) for f in fr]
    return ([(so, round(f * t), bo, round(g * nb)) for f, g in zip(fr, fr[::-1])]
            + [(so, round(0.8 * t), bo, round(0.7 * nb)), (so, t + 1, bo, nb + 1), (so, 0, bo, nb // 2)])


# triangular, odd m: the reference's neighbour table is not symmetric at the edges, and the
# site labeling follows the table while bond_list holds each pair once -- only the bond
# kind's components are the bond list's there (the positions hold for every m)
@pytest.mark.parametrize("lat,m,n,pbc,kind", [g + (k,) for g in GEOMS for k in KINDS
                                              if not (g[0] == 1 and g[1] % 2 and k != L.BOND)])
def test_geometry_equals_pairwise_sums(lat, m, n, pbc, kind):
    for so, ns, bo, nbc in cases(lat, m, n, kind):
        want, wrows = brute(lat, m, n, kind, so, ns, bo, nbc)
        rec, rows = api.cluster_geometry_host(lat, m, n, pbc, kind, so, ns, bo, nbc)
        assert {f: int(rec[f]) for f in FIELDS} == want, (ns, nbc)
        assert rows.tolist() == wrows, (ns, nbc)
        # the invariants: the spanning clusters are clusters, the rows sum to the record
        for a, b in (("span_n1", "n1"), ("span_n2", "n2"), ("span_g2", "g2"), ("root_n", "span_n1"),
                     ("root_g2", "span_g2"), ("big_g2", "g2")):
            assert 0 <= rec[a] <= rec[b]
        assert rows[32:64].sum() == rec["n2"] and rows[64:].sum() == rec["g2"]
        st, _ = api.cluster_stats_host(lat, m, n, pbc, kind, so, ns, bo, nbc)
        assert rows[:32].sum() == st["nclusters"] - st["nlone"]
        assert (rec["root_n"] > 0) == (st["nspan"] > 0) and (rec["span_n1"] > 0) == (st["nspan"] > 0)
        if kind == L.SITE:  # n_c is the size for the site kind only
            assert (rec["n1"], rec["n2"], rec["span_n2"]) == (st["s1"], st["s2"], st["span_s2"])
            assert rec["big_n"] == st["maxcs"] and rec["root_n"] == st["span_size"]


@pytest.mark.parametrize("lat,ms", [(0, range(3, 13)), (1, range(4, 13, 2))])
def test_every_bond_has_unit_length(lat, ms):
    for m in ms:
        for n in range(3, 12):
            b1, b2 = api.bond_list(lat, m, n, 0)
            x, y, wx, unit = api.site_positions(lat, m, n)
            dd = wx * (x[b1 - 1] - x[b2 - 1]) ** 2 + (y[b1 - 1] - y[b2 - 1]) ** 2
            assert (dd == unit).all(), (lat, m, n)
            assert unit == (4 if lat else 1)
            assert all(d2(lat, m, int(a) - 1, int(b) - 1) == unit for a, b in zip(b1[:50], b2[:50]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,n", [(3, 3), (12, 7), (50, 50), (128, 128), (3, 5461)])
def test_full_rectangle_closed_form(m, n, kind):
    """one cluster of every site: G = t^2 ((m^2 - 1) + (n^2 - 1)) / 12 on the
    square lattice (the variance of 0..k-1 is (k^2 - 1) / 12)"""
    t, nb = m * n, api.nbonds(0, m, n, 0)
    so, bo = np.arange(1, t + 2, dtype=np.int32), np.arange(1, nb + 2, dtype=np.int32)
    so[-1] = bo[-1] = 0
    rec, rows = api.cluster_geometry_host(0, m, n, 0, kind, so, t, bo, nb)
    G = t * t * ((m * m - 1) + (n * n - 1)) // 12
    assert (t * t * ((m * m - 1) + (n * n - 1))) % 12 == 0
    for f, v in dict(n1=t, span_n1=t, big_root=1, big_n=t, root_n=t, n2=t * t, span_n2=t * t, g2=G, span_g2=G,
                     big_g2=G, root_g2=G).items():
        assert int(rec[f]) == v, f
    b = t.bit_length() - 1
    assert (rows[b], rows[32 + b], rows[64 + b]) == (1, t * t, G) and rows.sum() == 1 + t * t + G
    if (m, n) == (128, 128):
        assert G > 2 ** 32 and (m * (m - 1) // 2 * n) ** 2 > 2 ** 32  # (sum c)^2 too: no 32-bit square


def test_mixed_lone_bonds_do_not_enter():
    lat, m, n = 0, 9, 8
    t, nb = m * n, api.nbonds(lat, m, n, 0)
    so, bo = api.shuffled_ids(t, 3), api.shuffled_ids(nb, 4)
    rec, rows = api.cluster_geometry_host(lat, m, n, 0, L.SITEBOND, so, 0, bo, nb // 2)
    st, _ = api.cluster_stats_host(lat, m, n, 0, L.SITEBOND, so, 0, bo, nb // 2)
    assert st["nlone"] == st["nclusters"] > 0
    assert rec == np.zeros((), dtype=L.GEOM_DTYPE) and not rows.any()
    # with sites: the bonds change which sites connect, never the member sites
    a, _ = api.cluster_geometry_host(lat, m, n, 0, L.SITEBOND, so, t // 2, bo, nb)
    b, _ = api.cluster_geometry_host(lat, m, n, 0, L.SITE, so, t // 2, None, 0)
    assert a == b and a["n1"] == t // 2


def test_empty_item_and_errors():
    rec, rows = api.cluster_geometry_host(1, 6, 5, 0, L.BOND, None, 0, api.shuffled_ids(api.nbonds(1, 6, 5, 0), 1), 0)
    assert rec == np.zeros((), dtype=L.GEOM_DTYPE) and not rows.any() and rows.dtype == np.int64
    with pytest.raises(ValueError, match="pbc"):
        api.cluster_geometry_host(0, 6, 5, 1, L.SITE, api.shuffled_ids(30, 1), 10)
    with pytest.raises(ValueError, match="kind"):
        api.cluster_geometry_host(0, 6, 5, 0, L.BONDSITE, api.shuffled_ids(30, 1), 10)
    with pytest.raises(ValueError, match="pbc"):
        api.correlation_curve(0, 6, 5, 1, L.SITE, grid=[0.5], batch=0)


def test_geometry_supported_is_clusters_supported_without_pbc():
    for lat, m, n in [(0, 3, 3), (0, 128, 128), (1, 128, 128), (1, 3, 5461), (0, 5461, 3), (1, 33, 31),
                      (0, 2, 50), (0, 129, 128), (0, 128, 129)]:
        for nexact in (0, 1024, 1025):
            assert api.batch_geometry_supported(lat, m, n, 0, nexact) == \
                api.batch_clusters_supported(lat, m, n, 0, nexact), (lat, m, n, nexact)
            assert not api.batch_geometry_supported(lat, m, n, 1, nexact)
    assert api.batch_geometry_supported(0, 128, 128, 0, 1024) and api.batch_geometry_supported(1, 3, 5461, 0, 1024)
    assert L.GEOM_DTYPE.itemsize == 72 and L.GEOM_ROW == 96


@pytest.mark.parametrize("kind", KINDS)
def test_correlation_curve_on_the_host(kind):
    grid = [(0.5, 0.9), (0.8, 0.7), (1.0, 1.0)] if kind == L.SITEBOND else [0.3, 0.55, 1.0]
    args = dict(lattice=1, m=8, n=7, pbc=0, kind=kind, grid=grid, master=58302, numtrials=3, nexact=16)
    r = api.correlation_curve(batch=0, **args)
    trials, stats, hist = api.cluster_curve(batch=0, **args)
    assert np.array_equal(r["stats"], stats) and np.array_equal(r["hist"], hist)
    assert r["unit"] == 4 and r["sums"].shape == (3, 10) and r["rows"].shape == (3, 96)
    # the rows of a trial are cluster_curve's plus the geometry record
    for tr, tg in zip(trials, r["trials"]):
        for a, b in zip(tr["rows"], tg["rows"]):
            assert a.items() <= b.items() and set(b) - set(a) == set(FIELDS)
    tot = np.zeros(10, dtype=np.int64)
    for tg in r["trials"]:
        q = tg["rows"][1]
        tot += [1] + [q[f] for f in api.GEOM_SUMS] + [q["big_n"] ** 2]
    assert np.array_equal(r["sums"][1], tot)
    # full occupancy: one spanning cluster, xi has no finite cluster to run over
    t = 56
    assert r["sums"][2].tolist()[:3] == [3, 3 * t, 3 * t * t] and np.isnan(r["xi"][2])
    g2 = r["sums"][2, 3] / 3
    assert r["big_r2"][2] == pytest.approx(g2 / (4 * t * t)) and r["rs2"][2, 5] == pytest.approx(g2 / (4 * t * t))
    s = r["sums"][1]
    if s[2] > s[5]:
        assert r["xi"][1] == pytest.approx(np.sqrt(2 * (s[3] - s[6]) / (4 * (s[2] - s[5]))))
