"""Structured occupancies for the labeling tests -- TEST INFRASTRUCTURE ONLY.

Uniform random occupation gives shallow union-find trees, short runs and at
most a cluster or two that span.  The patterns here are the opposite: rows
that are one run from edge to edge, stripes and combs whose crossing links
all join different clusters, serpentines and spirals that are one chain as
long as the lattice, and up to m / 2 spanning clusters at once.

Pure numpy over oracle_lib.bond_list(lat, m, n, pbc): site s (1-based) is in
row (s-1)//m and column (s-1)%m; row 0 is the bottom electrode, row n-1 the
top one.  A bond is horizontal when both ends share a row (the pbc wrap
bonds too; "no wrap" leaves them out) and vertical when both share a
column; the triangular lattice's diagonals belong to no bond pattern.  The
generators are the same for both lattices and for pbc -- what the partition
is, the oracle decides.  Each returns a sorted int32 array of 1-based ids.
"""
import functools

import numpy as np

import oracle_lib as O

ORDERS = ("asc", "desc", "perm")

# (lattice, m, n, pbc): the smallest lattices that cross every edge the
# labeling kernels have.  Open square: wave tiles of 128 x 16 (k_cc_tile_w,
# the square merge) -- one column / row past a tile, two and three tiles, a
# tile exactly, half a tile wide (no second column of a lane), a quarter tile
# high, and m > 2048 (three flags per thread in k_span_top).  The others: the
# 128 x 32 LDS union-find tiles and the generic merge.
SQ_OPEN = [(0, 129, 17, 0), (0, 257, 33, 0), (0, 300, 70, 0), (0, 64, 129, 0), (0, 130, 4, 0),
           (0, 128, 16, 0), (0, 2050, 20, 0)]
GENERIC = [(0, 129, 31, 1), (0, 384, 65, 1), (1, 130, 33, 0), (1, 256, 96, 1), (1, 64, 40, 1)]
GEOMS = SQ_OPEN + GENERIC
KINDS = ("bond", "site", "mixed")


@functools.lru_cache(maxsize=None)
def bonds(lat, m, n, pbc):
    """(b1, b2, r1, c1, r2, c2) of the bond list, 0-based rows / columns"""
    b1, b2 = O.bond_list(lat, m, n, pbc)
    for a in (b1, b2):
        a.setflags(write=False)
    s1, s2 = b1.astype(np.int64) - 1, b2.astype(np.int64) - 1
    return b1, b2, s1 // m, s1 % m, s2 // m, s2 % m


def _ids(mask):
    return (np.nonzero(mask)[0] + 1).astype(np.int32)


def _horiz(lat, m, n, pbc, wrap=True):
    _, _, r1, c1, r2, c2 = bonds(lat, m, n, pbc)
    h = r1 == r2
    return h if wrap else h & (np.abs(c1 - c2) == 1)


def _vert(lat, m, n, pbc):
    """(mask, lower row, column) of the vertical bonds"""
    _, _, r1, c1, r2, c2 = bonds(lat, m, n, pbc)
    return c1 == c2, np.minimum(r1, r2), c1


def _serp_col(r, m):
    """the serpentine's connector column between rows r and r + 1"""
    return np.where((r // 2) % 2 == 0, m - 1, 0)


def _path_bonds(lat, m, n, pbc, path):
    """ids of the bonds between consecutive sites (0-based) of a path"""
    b1, b2 = bonds(lat, m, n, pbc)[:2]
    t = m * n
    key = b1.astype(np.int64) * (t + 1) + b2
    order = np.argsort(key, kind="stable")
    p = np.asarray(path, dtype=np.int64) + 1
    lo, hi = np.minimum(p[:-1], p[1:]), np.maximum(p[:-1], p[1:])
    want = lo * (t + 1) + hi
    pos = np.searchsorted(key[order], want)
    assert np.array_equal(key[order][pos], want), "a path step is no bond of the lattice"
    return np.sort(order[pos] + 1).astype(np.int32)


# ---------------------------------------------------------------- bond patterns
def b_hstripes(lat, m, n, pbc):
    return _ids(_horiz(lat, m, n, pbc))


def b_hstripes_rungs(lat, m, n, pbc):
    E = [c for c in (0, 63, 64, 127, 128, m - 1) if c < m]
    v, r, c = _vert(lat, m, n, pbc)
    rung = v & (c == np.asarray(E)[r % len(E)])
    return _ids(_horiz(lat, m, n, pbc) | rung)


def b_vstripes(lat, m, n, pbc):
    v, _, c = _vert(lat, m, n, pbc)
    return _ids(v & (c % 2 == 0))


def _b_serp_mask(lat, m, n, pbc):
    r1 = bonds(lat, m, n, pbc)[2]
    v, r, c = _vert(lat, m, n, pbc)
    return (_horiz(lat, m, n, pbc, wrap=False) & (r1 % 2 == 0)) | (v & (c == _serp_col(r, m)))


def b_serp(lat, m, n, pbc):
    return _ids(_b_serp_mask(lat, m, n, pbc))


def b_serp_short(lat, m, n, pbc):
    """serp stopping short of the top row: without the vertical bonds into it
    (n even: the top row is a connector row); n odd: without every bond that
    touches the top two rows"""
    _, _, r1, _, r2, _ = bonds(lat, m, n, pbc)
    v, r, _ = _vert(lat, m, n, pbc)
    if n % 2 == 0:
        drop = v & (r == n - 2)
    else:
        drop = np.maximum(r1, r2) >= n - 2
    return _ids(_b_serp_mask(lat, m, n, pbc) & ~drop)


def b_vserp(lat, m, n, pbc):
    """serp transposed: the even columns' vertical bonds, joined along the
    top row (column pair c, c + 1 with c//2 even) or the bottom row"""
    _, _, r1, c1, _, c2 = bonds(lat, m, n, pbc)
    v, _, c = _vert(lat, m, n, pbc)
    cl = np.minimum(c1, c2)
    conn = _horiz(lat, m, n, pbc, wrap=False) & (r1 == np.where((cl // 2) % 2 == 0, n - 1, 0))
    return _ids((v & (c % 2 == 0)) | conn)


def _b_combs_mask(lat, m, n, pbc):
    r1 = bonds(lat, m, n, pbc)[2]
    h = _horiz(lat, m, n, pbc)
    v, r, c = _vert(lat, m, n, pbc)
    lower = (h & (r1 == 0)) | (v & (c % 2 == 0) & (r + 1 <= n - 2))
    upper = (h & (r1 == n - 1)) | (v & (c % 2 == 1) & (r >= 1))
    return lower | upper


def b_combs(lat, m, n, pbc):
    return _ids(_b_combs_mask(lat, m, n, pbc))


def b_combs_joined(lat, m, n, pbc):
    _, _, r1, c1, _, c2 = bonds(lat, m, n, pbc)
    link = _horiz(lat, m, n, pbc, wrap=False) & (r1 == n // 2) & (np.minimum(c1, c2) == m // 2)
    assert link.sum() == 1
    return _ids(_b_combs_mask(lat, m, n, pbc) | link)


def b_stair(lat, m, n, pbc):
    """(r, r) -> (r, r+1) -> (r+1, r+1) from the bottom left corner, while
    inside the lattice"""
    path = []
    r = 0
    while r < n and r < m:
        path.append(r * m + r)
        if r + 1 >= m:
            break
        path.append(r * m + r + 1)
        r += 1
    return _path_bonds(lat, m, n, pbc, path)


def b_spiral(lat, m, n, pbc):
    """one path from (0, 0) along the outer ring and inwards, counter-
    clockwise as drawn with row 0 at the bottom, arms two sites apart"""
    seen = np.zeros((n, m), dtype=bool)
    r = c = 0
    seen[0, 0] = True
    path = [0]
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    d = 0

    def free(rr, cc):
        return 0 <= rr < n and 0 <= cc < m and not seen[rr, cc]

    def ahead(dr, dc):
        rr, cc = r + dr, c + dc
        if not free(rr, cc):
            return False
        r2, c2 = rr + dr, cc + dc
        return not (0 <= r2 < n and 0 <= c2 < m and seen[r2, c2])

    while True:
        if not ahead(*dirs[d]):
            d = (d + 1) % 4
            if not ahead(*dirs[d]):
                break
        r, c = r + dirs[d][0], c + dirs[d][1]
        seen[r, c] = True
        path.append(r * m + c)
    return _path_bonds(lat, m, n, pbc, path)


BOND = {"hstripes": b_hstripes, "hstripes_rungs": b_hstripes_rungs, "vstripes": b_vstripes,
        "serp": b_serp, "serp_short": b_serp_short, "vserp": b_vserp, "combs": b_combs,
        "combs_joined": b_combs_joined, "stair": b_stair, "spiral": b_spiral}


# ---------------------------------------------------------------- site patterns
def _rc(m, n):
    s = np.arange(m * n, dtype=np.int64)
    return s // m, s % m


def s_hstripes(m, n):
    r, _ = _rc(m, n)
    return _ids(r % 2 == 0)


def s_vstripes(m, n):
    _, c = _rc(m, n)
    return _ids(c % 2 == 0)


def s_checker(m, n):
    r, c = _rc(m, n)
    return _ids((r + c) % 2 == 0)


def _s_serp_mask(m, n):
    r, c = _rc(m, n)
    return (r % 2 == 0) | (c == _serp_col(r, m))


def s_serp(m, n):
    return _ids(_s_serp_mask(m, n))


def s_serp_short(m, n):
    """serp stopping short of the top row: without the top row's connector
    site (n even); n odd: without the top two rows"""
    r, _ = _rc(m, n)
    return _ids(_s_serp_mask(m, n) & (r < (n - 1 if n % 2 == 0 else n - 2)))


def _s_combs_mask(m, n):
    r, c = _rc(m, n)
    return (r == 0) | ((c % 4 == 0) & (r <= n - 3)) | (r == n - 1) | ((c % 4 == 2) & (r >= 2))


def s_combs(m, n):
    return _ids(_s_combs_mask(m, n))


def s_combs_joined(m, n):
    r, c = _rc(m, n)
    c0 = 4 * (m // 8)
    return _ids(_s_combs_mask(m, n) | ((r == n // 2) & (c >= c0) & (c <= c0 + 2)))


SITE = {"hstripes": s_hstripes, "vstripes": s_vstripes, "checker": s_checker, "serp": s_serp,
        "serp_short": s_serp_short, "combs": s_combs, "combs_joined": s_combs_joined}

# mixed (site-then-bond) cases: (site pattern or None = every site, bond
# pattern or None = every bond)
MIXED = ([("s:" + k, k, None) for k in SITE] + [("b:" + k, None, k) for k in BOND]
         + [("s:vstripes*b:vstripes", "vstripes", "vstripes")])


@functools.lru_cache(maxsize=None)
def bond_ids(name, lat, m, n, pbc):
    nb = len(bonds(lat, m, n, pbc)[0])
    ids = np.arange(1, nb + 1, dtype=np.int32) if name is None else BOND[name](lat, m, n, pbc)
    assert len(ids) and np.all(np.diff(ids) > 0) and ids[0] >= 1 and ids[-1] <= nb
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def site_ids(name, m, n):
    ids = np.arange(1, m * n + 1, dtype=np.int32) if name is None else SITE[name](m, n)
    assert len(ids) and np.all(np.diff(ids) > 0) and ids[0] >= 1 and ids[-1] <= m * n
    ids.setflags(write=False)
    return ids


def ordered(ids, order, seed=0):
    """the id set ascending, descending, or in a seeded permutation"""
    if order == "asc":
        return np.ascontiguousarray(ids, dtype=np.int32)
    if order == "desc":
        return np.ascontiguousarray(ids[::-1], dtype=np.int32)
    assert order == "perm"
    return np.ascontiguousarray(ids[np.random.default_rng(seed).permutation(len(ids))], dtype=np.int32)


def order_row(head, N):
    """an order of N + 1 entries as the one-workgroup kernels read them: the
    ids `head` in the order given, the remaining ids ascending, the spill
    slot 0"""
    head = np.asarray(head, dtype=np.int32)
    rest = np.setdiff1d(np.arange(1, N + 1, dtype=np.int32), head)
    row = np.concatenate([head, rest, np.zeros(1, np.int32)]).astype(np.int32)
    assert len(row) == N + 1
    return row


def serp_connector_last(kind_name, lat, m, n, pbc, seed=5):
    """(order row, pattern length) of the bond / site serpentine with the
    rest of the chain shuffled and one connector half way up placed last: the
    chain is complete only with the pattern's final element"""
    r0 = 2 * (n // 4)
    if kind_name == "bond":
        ids = bond_ids("serp", lat, m, n, pbc)
        v, r, c = _vert(lat, m, n, pbc)
        conn = _ids(v & (r == r0) & (c == _serp_col(r, m)))
        N = len(v)
    else:
        ids = site_ids("serp", m, n)
        conn = np.array([(r0 + 1) * m + int(_serp_col(np.int64(r0 + 1), m)) + 1], dtype=np.int32)
        N = m * n
    assert len(conn) == 1 and conn[0] in ids
    head = ordered(ids[ids != conn[0]], "perm", seed)
    return order_row(np.concatenate([head, conn]), N), len(ids)


def cases(kind_name, lat, m, n, pbc):
    """[(name, site ids or None, bond ids or None)] of a kind ('bond', 'site',
    'mixed') on a lattice"""
    if kind_name == "bond":
        return [(k, None, bond_ids(k, lat, m, n, pbc)) for k in BOND]
    if kind_name == "site":
        return [(k, site_ids(k, m, n), None) for k in SITE]
    return [(k, site_ids(sp, m, n), bond_ids(bp, lat, m, n, pbc)) for k, sp, bp in MIXED]


# ---------------------------------------------------------------- the independent reference
def scipy_partition(lat, m, n, pbc, sids=None, bids=None):
    """canonical partition (minimum site of the component, 0 for a non-
    member) by scipy.sparse.csgraph.connected_components.  bids only: the
    bond rule (members are the occupied bonds' end sites); sids only: the
    site rule (every lattice bond between two occupied sites connects); both:
    the mixed rule (an occupied bond between two occupied sites connects;
    the members are the occupied sites)."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components

    b1, b2 = bonds(lat, m, n, pbc)[:2]
    t = m * n
    occ = np.ones(t, dtype=bool)
    if sids is not None:
        occ[:] = False
        occ[np.asarray(sids, dtype=np.int64) - 1] = True
    e = np.ones(len(b1), dtype=bool)
    if bids is not None:
        e[:] = False
        e[np.asarray(bids, dtype=np.int64) - 1] = True
    e &= occ[b1 - 1] & occ[b2 - 1]
    if sids is None:
        member = np.zeros(t, dtype=bool)
        member[b1[e] - 1] = True
        member[b2[e] - 1] = True
    else:
        member = occ
    g = sp.coo_matrix((np.ones(int(e.sum()), np.int8), (b1[e] - 1, b2[e] - 1)), shape=(t, t))
    _, comp = connected_components(g, directed=False)
    mins = np.full(comp.max() + 1, t + 1, dtype=np.int64)
    np.minimum.at(mins, comp, np.arange(1, t + 1))
    return np.where(member, mins[comp], 0).astype(np.int32)


def oracle_numbers(kind_name, lat, m, n, pbc, sorder=None, border=None):
    """the oracle's replay of an ordered occupancy, everything the tests
    compare: dict(canon, perccln, span_root, bond_label, site_label, csize,
    maxcs) -- the labels and perccln depend on the order, canon does not"""
    b1, b2 = bonds(lat, m, n, pbc)[:2]
    t, nb = m * n, len(b1)
    L = O.lib()
    bl = sl = None
    if border is not None:
        tb = len(border)
        o1, o2 = O.i32(nb + 1), O.i32(nb + 1)
        sel = np.asarray(border, dtype=np.int64) - 1
        o1[:tb], o2[:tb] = b1[sel], b2[sel]
    if sorder is not None:
        ts = len(sorder)
        so = O.i32(t + 1)
        so[:ts] = sorder
    if kind_name == "bond":
        bl, csize, cln, _, maxcs = O.label_bonds(lat, m, n, pbc, b1, b2, o1, o2, tb, literal=False)
        perccln = L.or_span_bonds(m, n, nb, b1, b2, bl, csize, cln)
        canon = O.canon_bonds(t, b1, b2, bl, cln)
        root = int(canon[b1[np.nonzero(bl == perccln)[0][0]] - 1]) if perccln > 0 else 0
    elif kind_name == "site":
        sl, csize, cln, _, maxcs = O.label_sites(lat, m, n, pbc, so, ts, literal=False)
        perccln = L.or_span_sites(m, n, sl, csize, cln, n)
        canon = O.canon_sites(sl, cln)
        root = int(canon[np.nonzero(sl == perccln)[0][0]]) if perccln > 0 else 0
    else:
        sl, bl, csize, cln, _, maxcs = O.label_sitebond(lat, m, n, pbc, b1, b2, so, ts, o1, o2, tb,
                                                        literal=False)
        perccln = L.or_span_sites(m, n, sl, csize, cln, 2 * n - 1)
        canon = O.canon_sites(sl, cln)
        root = int(canon[np.nonzero(sl == perccln)[0][0]]) if perccln > 0 else 0
    return dict(canon=canon, perccln=int(perccln), span_root=root, bond_label=bl, site_label=sl,
                csize=csize, maxcs=int(maxcs))


def spanning_roots(canon, m, n):
    """the roots (canonical ids <= m: clusters with a bottom-row member) of
    the top row's members, ascending"""
    top = canon[(n - 1) * m:]
    return np.unique(top[(top > 0) & (top <= m)])
