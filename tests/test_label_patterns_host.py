"""The structured occupancies of label_patterns.py on the CPU: what the GPU
tests of test_label_patterns.py compare against is pinned here first.

For every pattern, geometry and order the oracle's replay partition
(oracle/perc_oracle.c, as test_labeling_oracle.py's helpers read it) equals
an independent scipy.sparse.csgraph.connected_components partition and does
not depend on the order; on the open square lattice the patterns are what
their names say (cluster counts and spanning verdicts stated from the scipy
side alone, so the GPU tests cannot pass on degenerate inputs); the stripes
straddle k_span_top's list of kMaxSpanList = 64 spanning roots; and
libperc's own host replay (perc_replay_labels) numbers the clusters as the
oracle does, in all three orders.
"""
import numpy as np
import pytest

import label_patterns as LP
from percolation_amd import _lib as PL
from percolation_amd import api
from test_labeling_oracle import oracle_bond, oracle_mixed, oracle_site

KIND = {"bond": PL.BOND, "site": PL.SITE, "mixed": PL.SITEBOND}


def reused_oracle(kind_name, lat, m, n, pbc, so, bo):
    """(canon, perccln, span_root) by test_labeling_oracle's own helpers"""
    if kind_name == "bond":
        return oracle_bond(lat, m, n, pbc, bo, len(bo))
    if kind_name == "site":
        return oracle_site(lat, m, n, pbc, so, len(so))
    return oracle_mixed(lat, m, n, pbc, so, len(so), bo, len(bo))


def nclusters(canon):
    return len(np.unique(canon[canon > 0]))


# ---------------------------------------------------------------- threshold scans
# the one-workgroup kernels' lattices: the reference's own 50 x 50, 128 x 64
# (near perc_batch_cond_supported's 8192 interior rows), 128 x 128
# (perc_scan_supported's limit; scans only), open and pbc, and a triangular one
BATCH_COND = [(0, 50, 50, 0), (0, 50, 50, 1), (0, 128, 64, 0), (0, 128, 64, 1), (1, 64, 40, 1)]
BATCH_SCAN = BATCH_COND + [(0, 128, 128, 0), (0, 128, 128, 1)]


def oracle_first(spans, N):
    """perc_first_spanning's bisection with the oracle's spanning test"""
    if not spans(N):
        return 0
    lo, hi = 0, N
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if spans(mid):
            hi = mid
        else:
            lo = mid
    return hi


_SCANS = {}


def scan_cases(geom):
    """the scan trials of a lattice, each with the oracle's first spanning
    count: [dict(name, kind, scan, so, bo, fixed, length, first)], computed
    once.  length: the pattern's own length (the head of the scanned row)."""
    if geom in _SCANS:
        return _SCANS[geom]
    lat, m, n, pbc = geom
    t, nb = m * n, len(LP.bonds(lat, m, n, pbc)[0])
    out = []
    for kind_name, N in (("bond", nb), ("site", t)):
        row, k = LP.serp_connector_last(kind_name, lat, m, n, pbc)
        ids = (LP.bond_ids("serp_short", lat, m, n, pbc) if kind_name == "bond"
               else LP.site_ids("serp_short", m, n))
        for name, r, length in ((kind_name + " serp, a connector last", row, k),
                                (kind_name + " serp_short, then the rest",
                                 LP.order_row(LP.ordered(ids, "desc"), N), len(ids))):
            if kind_name == "bond":
                first = oracle_first(lambda c: oracle_bond(lat, m, n, pbc, r, c)[1] > 0, N)
                out.append(dict(name=name, kind=PL.BOND, scan=PL.BOND, so=None, bo=r, fixed=None,
                                length=length, first=first))
            else:
                first = oracle_first(lambda c: oracle_site(lat, m, n, pbc, r, c)[1] > 0, N)
                out.append(dict(name=name, kind=PL.SITE, scan=PL.BOND, so=r, bo=None, fixed=None,
                                length=length, first=first))
    sv, bv = LP.site_ids("vstripes", m, n), LP.bond_ids("vstripes", lat, m, n, pbc)
    so, bo = LP.order_row(sv, t), LP.order_row(bv, nb)
    first = oracle_first(lambda c: oracle_mixed(lat, m, n, pbc, so, len(sv), bo, c)[1] > 0, nb)
    out.append(dict(name="site vstripes fixed, bonds vstripes first", kind=PL.SITEBOND, scan=PL.BOND,
                    so=so, bo=bo, fixed=len(sv), length=len(bv), first=first))
    first = oracle_first(lambda c: oracle_mixed(lat, m, n, pbc, so, c, bo, len(bv))[1] > 0, t)
    out.append(dict(name="bond vstripes fixed, sites vstripes first", kind=PL.SITEBOND, scan=PL.SITE,
                    so=so, bo=bo, fixed=len(bv), length=len(sv), first=first))
    _SCANS[geom] = out
    return out


@pytest.mark.parametrize("geom", BATCH_SCAN)
def test_scan_orders_on_the_cpu(geom):
    """the serpentine with a connector last spans with its final element and
    not before; the stripes' mixed scans span within the stripes' own prefix
    (the first even column completes there)"""
    sc = {c["name"]: c for c in scan_cases(geom)}
    assert len(sc) == 6
    for kind_name in ("bond", "site"):
        c = sc[kind_name + " serp, a connector last"]
        assert c["first"] == c["length"], (c["name"], c["first"], c["length"])
        c = sc[kind_name + " serp_short, then the rest"]
        assert c["first"] > c["length"], (c["name"], c["first"], c["length"])
    for name in ("site vstripes fixed, bonds vstripes first", "bond vstripes fixed, sites vstripes first"):
        assert 0 < sc[name]["first"] <= sc[name]["length"], (name, sc[name]["first"])


@pytest.mark.parametrize("geom", LP.GEOMS)
@pytest.mark.parametrize("kind_name", LP.KINDS)
def test_oracle_partition_equals_scipy_in_every_order(geom, kind_name):
    lat, m, n, pbc = geom
    for name, sids, bids in LP.cases(kind_name, lat, m, n, pbc):
        want = LP.scipy_partition(lat, m, n, pbc, sids, bids)
        for k, order in enumerate(LP.ORDERS):
            so = None if sids is None else LP.ordered(sids, order, 11 + k)
            bo = None if bids is None else LP.ordered(bids, order, 23 + k)
            tag = (name, order)
            canon, perccln, span_root = reused_oracle(kind_name, lat, m, n, pbc, so, bo)
            assert np.array_equal(canon, want), tag
            roots = LP.spanning_roots(want, m, n)
            assert (perccln > 0) == (len(roots) > 0), tag
            if perccln > 0:
                assert span_root in roots, tag
            # the one replay the GPU tests take label numbers and sizes from
            on = LP.oracle_numbers(kind_name, lat, m, n, pbc, so, bo)
            assert np.array_equal(on["canon"], canon), tag
            assert (on["perccln"], on["span_root"]) == (perccln, span_root), tag
            lab = on["site_label"] if kind_name == "site" else on["bond_label"]
            if kind_name != "mixed":
                assert on["maxcs"] == on["csize"][np.unique(lab[lab > 0])].max(), tag
            # libperc's host replay: the same numbering
            r = api.replay_labels(lat, m, n, pbc, KIND[kind_name], site_order=so,
                                  nsites=0 if so is None else len(so), bond_order=bo,
                                  nbond=0 if bo is None else len(bo))
            for key in ("bond_label", "site_label"):
                if on[key] is not None:
                    assert np.array_equal(r[key], on[key]), tag + (key,)
            assert r["perccln"] == perccln, tag
            assert r["maxcs"] == on["maxcs"], tag


@pytest.mark.parametrize("geom", LP.SQ_OPEN)
def test_patterns_are_what_their_names_say(geom):
    """open square lattice, from the scipy partition alone"""
    lat, m, n, pbc = geom
    t = m * n

    def part(kind_name, name):
        sids = LP.site_ids(name, m, n) if kind_name == "site" else None
        bids = LP.bond_ids(name, lat, m, n, pbc) if kind_name == "bond" else None
        canon = LP.scipy_partition(lat, m, n, pbc, sids, bids)
        return canon, nclusters(canon), len(LP.spanning_roots(canon, m, n))

    assert part("bond", "hstripes")[1:] == (n, 0)
    assert part("site", "hstripes")[1:] == ((n + 1) // 2, 0)
    for kind_name in ("bond", "site"):
        assert part(kind_name, "vstripes")[1:] == ((m + 1) // 2, (m + 1) // 2), kind_name
        for name in ("serp", "combs_joined"):
            assert part(kind_name, name)[1:] == (1, 1), (kind_name, name)
        assert part(kind_name, "serp_short")[1:] == (1, 0), kind_name
        assert part(kind_name, "combs")[1:] == (2, 0), kind_name
    for name in ("hstripes_rungs", "vserp", "spiral"):
        assert part("bond", name)[1:] == (1, 1), name
    canon, nc, nsp = part("bond", "stair")
    assert nc == 1 and nsp == (1 if m >= n else 0)
    canon, nc, nsp = part("site", "checker")
    assert nc == (t + 1) // 2 and nsp == 0
    assert np.array_equal(canon[canon > 0], np.nonzero(canon)[0] + 1)  # (every cluster one site)
    # one chain as long as the lattice: the serpentine holds every even row
    assert np.count_nonzero(part("bond", "serp")[0]) >= ((n + 1) // 2) * m


@pytest.mark.parametrize("lat,m,n,pbc,kinds,nspan", [
    (0, 129, 31, 1, ("site",), 64), (0, 129, 17, 0, ("bond", "site"), 65),
    (1, 130, 33, 0, ("bond", "site"), 65), (0, 300, 70, 0, ("bond", "site"), 150),
    (0, 2050, 20, 0, ("bond", "site"), 1025)])
def test_stripes_straddle_the_spanning_root_list(lat, m, n, pbc, kinds, nspan):
    """vstripes: 64, 65, 150 and 1025 spanning clusters (kMaxSpanList = 64;
    m = 2050 gives each of k_span_top's threads three flags)"""
    for kind_name in kinds:
        sids = LP.site_ids("vstripes", m, n) if kind_name == "site" else None
        bids = LP.bond_ids("vstripes", lat, m, n, pbc) if kind_name == "bond" else None
        canon = LP.scipy_partition(lat, m, n, pbc, sids, bids)
        assert len(LP.spanning_roots(canon, m, n)) == nspan, kind_name
