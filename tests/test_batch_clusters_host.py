"""The cluster table's statistics on the host: api.cluster_stats_host (the
reference every GPU test of Context.batch_clusters compares with) against
scipy's connected components and a direct count, the invariants of the
record and the histogram row, replay_labels' csize, the host-only predicate
perc_batch_clusters_supported and cluster_curve(batch=0).  No device."""
import inspect

import numpy as np
import pytest
import scipy.ndimage
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from percolation_amd import _lib as L
from percolation_amd import api

GEOMS = [(0, 7, 5, 0), (0, 7, 5, 1), (0, 12, 9, 0), (0, 12, 9, 1), (1, 8, 6, 0)]
KINDS = [L.BOND, L.SITE, L.SITEBOND]
NEXACT = 12


def occupied(order, count):
    ids = np.asarray(order[:count])
    return ids[ids > 0]


def direct_sizes(lat, m, n, pbc, kind, sids, bids):
    """[(size, min member site or 0, spans)] of every cluster, by scipy's
    components and a direct count of the mixed kind's bonds"""
    b1, b2 = api.bond_list(lat, m, n, pbc)
    t, nb = m * n, len(b1)
    socc = np.ones(t + 1, dtype=bool)
    bocc = np.ones(nb, dtype=bool)
    if kind != L.BOND:
        socc[:] = False
        socc[sids] = True
    if kind != L.SITE:
        bocc[:] = False
        bocc[bids - 1] = True
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
    size = {}
    for s in np.nonzero(member)[0]:
        if kind != L.BOND:
            size[comp[s]] = size.get(comp[s], 0) + 1
        else:
            size.setdefault(comp[s], 0)
    lone = 0
    if kind != L.SITE:
        for k in np.nonzero(bocc)[0]:
            a, b = b1[k], b2[k]
            if kind == L.BOND or socc[a]:
                size[comp[a]] += 1
            elif socc[b]:
                size[comp[b]] += 1
            else:
                lone += 1
    out = []
    for c, sz in size.items():
        sites = np.nonzero(member & (comp == c))[0]
        out.append((sz, int(sites.min()), bool((sites <= m).any() and (sites > t - m).any())))
    return out + [(1, 0, False)] * lone, lone


def expect(clusters, lone, nexact):
    rec = dict(nclusters=len(clusters), nlone=lone, nspan=0, span_root=0, span_size=0, maxcs=0, s1=0, s2=0,
               span_s1=0, span_s2=0)
    hist = np.zeros(nexact + 32, dtype=np.int64)
    root = None
    for sz, mn, spans in clusters:
        rec["s1"] += sz
        rec["s2"] += sz * sz
        rec["maxcs"] = max(rec["maxcs"], sz)
        if sz <= nexact:
            hist[sz - 1] += 1
        hist[nexact + sz.bit_length() - 1] += 1
        if spans:
            rec["nspan"] += 1
            rec["span_s1"] += sz
            rec["span_s2"] += sz * sz
            if root is None or mn < root:
                root, rec["span_root"], rec["span_size"] = mn, mn, sz
    return rec, hist


def counts_of(order, N):
    pos0 = int(np.nonzero(order == 0)[0][0])
    return [0, 1, N // 2, N, min(pos0 + 1, N + 1), N + 1]


def items(lat, m, n, pbc, kind, seed=4711):
    """(site order, nsites, bond order, nbonds) of the cases of one lattice
    and kind: counts 0, 1, about half, all, one that just covers the spill
    slot, the whole order"""
    t, nb = m * n, api.nbonds(lat, m, n, pbc)
    so, bo = api.shuffled_ids(t, seed), api.shuffled_ids(nb, seed + 1)
    if kind == L.BOND:
        return [(None, 0, bo, c) for c in counts_of(bo, nb)]
    if kind == L.SITE:
        return [(so, c, None, 0) for c in counts_of(so, t)]
    cs, cb = counts_of(so, t), counts_of(bo, nb)
    return ([(so, a, bo, b) for a, b in zip(cs, cb)]
            + [(so, 0, bo, nb // 2), (so, t // 2, bo, 0), (so, t // 3, bo, nb), (so, t, bo, nb // 3)])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lat,m,n,pbc", GEOMS)
def test_stats_equal_scipy_components(lat, m, n, pbc, kind):
    for so, ns, bo, nbc in items(lat, m, n, pbc, kind):
        sids = occupied(so, ns) if so is not None else None
        bids = occupied(bo, nbc) if bo is not None else None
        clusters, lone = direct_sizes(lat, m, n, pbc, kind, sids, bids)
        want, whist = expect([(int(a), b, c) for a, b, c in clusters], lone, NEXACT)
        rec, hist = api.cluster_stats_host(lat, m, n, pbc, kind, so, ns, bo, nbc, NEXACT)
        got = {f: int(rec[f]) for f in L.CLUSTER_DTYPE.names}
        assert got == want, (ns, nbc)
        assert np.array_equal(hist, whist), (ns, nbc)
        # the invariants
        s1 = {L.BOND: len(bids) if bids is not None else 0, L.SITE: len(sids) if sids is not None else 0}
        s1[L.SITEBOND] = s1[L.BOND] + s1[L.SITE]
        assert got["s1"] == s1[kind]
        assert hist[NEXACT:].sum() == got["nclusters"]
        # the exact part against the octaves wherever an octave lies inside it
        for k in range(32):
            lo, hi = 1 << k, (2 << k) - 1
            if hi <= NEXACT:
                assert hist[lo - 1:hi].sum() == hist[NEXACT + k]
        if kind != L.SITEBOND:
            assert got["nlone"] == 0


def test_site_kind_equals_ndimage_label():
    """the open square lattice's site clusters are scipy.ndimage's 4-connected
    components of the occupancy image"""
    m, n = 12, 9
    so = api.shuffled_ids(m * n, 99)
    for ns in (30, 54, 64, 90):
        img = np.zeros(m * n, dtype=bool)
        img[occupied(so, ns) - 1] = True
        lab, k = scipy.ndimage.label(img.reshape(n, m))
        sizes = np.sort(np.bincount(lab.ravel())[1:])
        rec, hist = api.cluster_stats_host(0, m, n, 0, L.SITE, so, ns, None, 0, 108)
        assert rec["nclusters"] == k and rec["maxcs"] == sizes[-1] and rec["s2"] == (sizes ** 2).sum()
        assert np.array_equal(np.repeat(np.arange(1, 109), hist[:108]), sizes)
        rows = [set(lab.reshape(n, m)[r]) - {0} for r in (0, n - 1)]
        assert rec["nspan"] == len(rows[0] & rows[1])


@pytest.mark.parametrize("kind", KINDS)
def test_csize_nonzero_entries_are_the_sizes(kind):
    """replay_labels' csize holds the same sizes, plus one phantom 1 where the
    spill slot lies inside a count of a list that opens a label for it"""
    lat, m, n, pbc = 0, 12, 9, 0
    t, nb = m * n, api.nbonds(lat, m, n, pbc)
    for so, ns, bo, nbc in items(lat, m, n, pbc, kind):
        if ns > t or nbc > nb:
            continue  # (replay_labels takes prefixes of at most N entries)
        r = api.replay_labels(lat, m, n, pbc, kind, site_order=so, nsites=ns, bond_order=bo, nbond=nbc)
        rec, hist = api.cluster_stats_host(lat, m, n, pbc, kind, so, ns, bo, nbc, 1024)
        assert hist[1024:].sum() == hist[:1024].sum()  # (every size below 1024 here)
        sizes = np.repeat(np.arange(1, 1025), hist[:1024])
        phantom = {L.BOND: int(0 in bo[:nbc]) if bo is not None else 0, L.SITE: 0,
                   L.SITEBOND: int(0 in so[:ns]) if so is not None else 0}[kind]
        cs = np.sort(r["csize"][r["csize"] > 0])
        assert np.array_equal(cs, np.sort(np.concatenate([sizes, np.ones(phantom, np.int64)]))), (ns, nbc)


@pytest.mark.parametrize("lat,m,n,pbc", [(0, 128, 128, 0), (1, 128, 128, 1), (0, 50, 50, 0), (1, 5, 3, 0),
                                         (0, 129, 128, 0), (1, 128, 129, 0), (0, 2, 50, 0)])
def test_clusters_supported(lat, m, n, pbc):
    scan = api.scan_supported(lat, m, n, pbc)
    for nexact in (0, 1, 64, 1024):
        assert api.batch_clusters_supported(lat, m, n, pbc, nexact) is scan
        assert L.lib().perc_batch_clusters_supported(lat, m, n, pbc, nexact) == int(scan)
    for nexact in (-1, 1025, 1 << 20):
        assert api.batch_clusters_supported(lat, m, n, pbc, nexact) is False
    assert scan == (m * n <= 16384 and m >= 3)


def test_clusters_symbols_and_signature():
    lib = L.lib()
    for name in ("perc_batch_clusters", "perc_batch_clusters_seeded", "perc_batch_clusters_supported"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert L.SIGNATURES["perc_batch_clusters"][1] == L.SIGNATURES["perc_batch_clusters_seeded"][1]
    p = inspect.signature(api.Context.batch_clusters).parameters
    assert list(p)[1:3] == ["kind", "item_trial"]
    assert p["nexact"].default == 0 and p["site_seeds"].default is None and p["bond_seeds"].default is None


@pytest.mark.parametrize("kind", KINDS)
def test_cluster_curve_host_sums_the_items(kind):
    """cluster_curve(batch=0) runs without a device: its statistics are the
    sums of the per-item records over the trials"""
    lat, m, n, pbc, nexact, master = 0, 10, 10, 0, 16, 58302
    t, nb = m * n, api.nbonds(lat, m, n, pbc)
    grid = ([(0.3, 0.9), (0.6, 0.6), (0.8, 0.5), (1.0, 1.0)] if kind == L.SITEBOND else [0.2, 0.5, 0.65, 1.0])
    trials, stats, hist = api.cluster_curve(lat, m, n, pbc, kind, grid, master, numtrials=3, batch=0,
                                            nexact=nexact)
    assert stats.shape == (4, 8) and stats.dtype == np.int64 and hist.shape == (4, nexact + 32)
    assert [tr["ii"] for tr in trials] == [1, 2, 3]
    if kind == L.SITEBOND:
        ss, bs = api.paired_seeds(master, 3)
    else:
        ss = bs = api.trial_seeds(master, 3)
    want = np.zeros((4, 8), dtype=np.int64)
    whist = np.zeros((4, nexact + 32), dtype=np.int64)
    for ii in range(3):
        so = api.shuffled_ids(t, int(ss[ii])) if kind != L.BOND else None
        bo = api.shuffled_ids(nb, int(bs[ii])) if kind != L.SITE else None
        for j, p in enumerate(grid):
            ps, pb = p if kind == L.SITEBOND else (p, p)
            rec, row = api.cluster_stats_host(lat, m, n, pbc, kind, so, int(ps * t), bo, int(pb * nb), nexact)
            want[j] += [1, rec["nclusters"], rec["nspan"] > 0, rec["span_size"], rec["s1"], rec["s2"],
                        rec["span_s1"], rec["span_s2"]]
            whist[j] += row
            assert {f: trials[ii]["rows"][j][f] for f in L.CLUSTER_DTYPE.names} == \
                {f: int(rec[f]) for f in L.CLUSTER_DTYPE.names}
    assert np.array_equal(stats, want) and np.array_equal(hist, whist)
    assert stats[:, 0].tolist() == [3] * 4 and stats[-1, 2] == 3  # (the full lattice spans)
