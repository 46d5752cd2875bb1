"""The bond-current record on the host (perc_current_stats_host,
api.current_stats_host, api.conducting_bonds; include/perc.h,
perc_batch_currents), without a device:

* on four lattices a bond occupancy is drawn, its spanning component found
  with scipy, the Kirchhoff system (g0 on the component's occupied bonds, the
  leak on every other bond) built in numpy and solved directly; the record of
  those voltages equals a plain numpy restatement of the definition -- the
  counts, the maximum and the histogram exactly, the sums within
  (nbonds + 8) 2^-52 relative (the host sums nbonds terms in bond-id order,
  numpy pairwise: each within (nbonds - 1) 2^-53 of the exact sum of the same
  terms);
* no current exceeds g0 Va, and the dissipated power of all bonds equals
  Itop Va (non-unit Va and g0);
* api.conducting_bonds' three rules on a hand-made 4 x 4 case;
* every PERC_EINVAL case decided without a context, and the entry points in
  the library, the header, the Fortran module and SIGNATURES."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components
from scipy.sparse.linalg import spsolve

from percolation_amd import _lib as L
from percolation_amd import api

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICES = [(0, 10, 10, 0), (0, 12, 11, 1), (1, 10, 10, 0), (1, 12, 10, 1)]
VALUES = [(1.0, 1.0, 1e-12), (2.5, 0.75, 1e-9)]  # (Va, g0, leak)
CUT = 1e-6
SUM_KEYS = ("s1", "s2", "s4", "s6")


def bar1(nbonds):
    return (nbonds + 8) * 2.0 ** -52


_SOLVED = {}


def solved(lat, vals):
    """a drawn bond occupancy of the lattice, its lowest spanning component's
    conducting mask, and the direct solve's interior voltages (computed once)"""
    if (lat, vals) in _SOLVED:
        return _SOLVED[lat, vals]
    lattice, m, n, pbc = lat
    Va, g0, leak = vals
    t = m * n
    b1, b2 = api.bond_list(*lat)
    nb = len(b1)
    rng = np.random.default_rng(1000 * lattice + 10 * m + pbc)
    occ = rng.random(nb) < (0.62 if lattice == 0 else 0.45)
    a, b = b1[occ] - 1, b2[occ] - 1
    ncomp, comp = connected_components(sp.coo_matrix((np.ones(len(a)), (a, b)), shape=(t, t)), directed=False)
    member = np.zeros(t, bool)
    member[a] = member[b] = True
    span = sorted(set(comp[:m][member[:m]]) & set(comp[t - m:][member[t - m:]]),
                  key=lambda c: np.nonzero(comp == c)[0][0])
    assert span, "the drawn occupancy must span"
    mask = occ & (comp[b1 - 1] == span[0])
    g = np.where(mask, g0, leak)
    # interior system: row s - m - 1 of site s, electrodes on the right-hand side
    N = t - 2 * m
    A = sp.lil_matrix((N, N))
    rhs = np.zeros(N)
    for k in range(nb):
        for s, c in ((b1[k], b2[k]), (b2[k], b1[k])):
            if m < s <= t - m:
                A[s - m - 1, s - m - 1] += g[k]
                if m < c <= t - m:
                    A[s - m - 1, c - m - 1] -= g[k]
                elif c > t - m:
                    rhs[s - m - 1] += g[k] * Va
    x = spsolve(sp.csc_matrix(A), rhs)
    V = np.concatenate([np.zeros(m), x, np.full(m, Va)])
    _SOLVED[lat, vals] = dict(b1=b1, b2=b2, mask=mask.astype(np.uint8), g=g, x=x, V=V)
    return _SOLVED[lat, vals]


def restate(lat, mask, x, Va, g0, cut):
    """the definition in plain numpy: (|i| of the counted bonds in id order,
    nbonds, nabove, imax, hist)"""
    lattice, m, n, pbc = lat
    t = m * n
    b1, b2 = api.bond_list(*lat)
    V = np.concatenate([np.zeros(m), np.asarray(x, dtype=np.float64), np.full(m, float(Va))])
    inner = lambda s: (s > m) & (s <= t - m)
    take = (np.asarray(mask) != 0) & (inner(b1) | inner(b2))
    a = np.abs(g0 * (V[b2[take] - 1] - V[b1[take] - 1]))
    imax = a.max() if len(a) else 0.0
    e0 = int(np.frexp(g0 * Va)[1]) - 1
    bins = np.full(len(a), 63, dtype=np.int64)
    nz = a != 0
    bins[nz] = np.clip(e0 - (np.frexp(a[nz])[1].astype(np.int64) - 1), 0, 63)
    return a, len(a), int(np.count_nonzero(a >= cut * imax)), float(imax), np.bincount(bins, minlength=64)


def check_record(rec, lat, mask, x, Va, g0, cut):
    """rec against the numpy restatement: ints, imax and hist exactly, the sums
    within bar 1; returns |i|"""
    a, nbonds, nabove, imax, hist = restate(lat, mask, x, Va, g0, cut)
    assert rec["nbonds"] == nbonds and rec["nabove"] == nabove and rec["imax"] == imax, (rec, nbonds, nabove, imax)
    assert (rec["hist"] == hist).all() and rec["hist"].sum() == rec["nbonds"]
    i2 = a * a
    i4 = i2 * i2
    for k, terms in zip(SUM_KEYS, (a, i2, i4, i4 * i2)):
        want = float(np.sum(terms))
        assert abs(rec[k] - want) <= bar1(nbonds) * want, (k, rec[k], want)
    return a


@pytest.mark.parametrize("vals", VALUES, ids=["unit", "nonunit"])
@pytest.mark.parametrize("lat", LATTICES)
def test_record_is_the_definition(lat, vals):
    Va, g0, leak = vals
    d = solved(lat, vals)
    for cut in (CUT, 0.0, 0.25, 1.0):
        rec = api.current_stats_host(*lat, d["mask"], d["x"], Va, g0, cut)
        a = check_record(rec, lat, d["mask"], d["x"], Va, g0, cut)
    assert rec["nbonds"] > 20 and rec["imax"] > 0.0
    assert (a <= g0 * Va * (1 + 1e-12)).all()
    # cut = 0 takes every bond, cut = 1 the bonds at the maximum
    assert api.current_stats_host(*lat, d["mask"], d["x"], Va, g0, 0.0)["nabove"] == rec["nbonds"]
    assert rec["nabove"] == np.count_nonzero(a == a.max())  # (the loop's last cut: 1.0)
    # a record without a conducting bond is all zero
    zero = api.current_stats_host(*lat, np.zeros_like(d["mask"]), d["x"], Va, g0, CUT)
    assert all(zero[k] == 0 for k in L.CURRENTS_KEYS[:-1]) and not zero["hist"].any()


@pytest.mark.parametrize("lat", LATTICES)
def test_power_identity(lat):
    """sum g dV^2 over all bonds, the leak ones included, = Itop Va to 1e-9
    relative (both sides from the direct solve; the conducting bonds' share is
    the record's s2 / g0).  Observed worst on these four systems: 2e-14."""
    vals = VALUES[1]
    Va, g0, leak = vals
    d = solved(lat, vals)
    lattice, m, n, pbc = lat
    t = m * n
    b1, b2, g, V = d["b1"], d["b2"], d["g"], d["V"]
    dv = V[b2 - 1] - V[b1 - 1]
    power = float(np.sum(g * dv * dv))
    top1, top2 = b1 > t - m, b2 > t - m
    itop = float(np.sum(g[top2 & ~top1] * dv[top2 & ~top1]) - np.sum(g[top1 & ~top2] * dv[top1 & ~top2]))
    print("lattice %s: power %.17g, Itop Va %.17g, relative %.3e" % (lat, power, itop * Va, abs(power / (itop * Va) - 1)))
    assert itop > 0 and abs(power - itop * Va) <= 1e-9 * itop * Va
    rec = api.current_stats_host(*lat, d["mask"], d["x"], Va, g0, CUT)
    cond = d["mask"] != 0
    leak_part = float(np.sum(g[~cond] * dv[~cond] * dv[~cond]))
    assert abs(rec["s2"] / g0 + leak_part - itop * Va) <= 1e-9 * itop * Va


def pairs_mask(b1, b2, pairs):
    want = np.zeros(len(b1), np.uint8)
    for p, q in pairs:
        k = np.nonzero((b1 == p) & (b2 == q))[0]
        assert len(k) == 1, (p, q)
        want[k[0]] = 1
    return want


def test_conducting_bonds_three_rules():
    """4 x 4 open square lattice, sites 1..16 row by row: column 0 (1, 5, 9,
    13) spans under every rule"""
    b1, b2 = api.bond_list(0, 4, 4, 0)
    occ_of = lambda ids, n: np.isin(np.arange(1, n + 1), ids).astype(np.uint8)
    canon_of = lambda d: np.array([d.get(s, 0) for s in range(1, 17)], np.int32)
    col = [(1, 5), (5, 9), (9, 13)]
    # BOND: the occupied bonds of the root's cluster, whatever the sites say
    bocc = pairs_mask(b1, b2, col + [(5, 6), (4, 8), (11, 12)])
    canon = canon_of({1: 1, 5: 1, 9: 1, 13: 1, 6: 1, 4: 4, 8: 4, 11: 11, 12: 11})
    got = api.conducting_bonds(L.BOND, b1, b2, np.zeros(16, np.uint8), bocc, canon, 1)
    assert (got == pairs_mask(b1, b2, col + [(5, 6)])).all() and got.dtype == np.uint8
    assert (api.conducting_bonds(L.BOND, b1, b2, np.zeros(16, np.uint8), bocc, canon, 4)
            == pairs_mask(b1, b2, [(4, 8)])).all()
    assert not api.conducting_bonds(L.BOND, b1, b2, np.zeros(16, np.uint8), bocc, canon, 0).any()
    # SITE: every bond between two occupied sites of the cluster, whatever the bonds say
    socc = occ_of([1, 5, 9, 13, 2, 4, 8], 16)
    canon = canon_of({1: 1, 2: 1, 5: 1, 9: 1, 13: 1, 4: 4, 8: 4})
    got = api.conducting_bonds(L.SITE, b1, b2, socc, np.zeros(len(b1), np.uint8), canon, 1)
    assert (got == pairs_mask(b1, b2, col + [(1, 2)])).all()
    # SITEBOND: the bond and both end sites (site 6 is empty, bond (1, 2) is not occupied)
    bocc = pairs_mask(b1, b2, col + [(5, 6), (4, 8)])
    canon = canon_of({1: 1, 5: 1, 9: 1, 13: 1, 2: 2, 4: 4, 8: 4})
    got = api.conducting_bonds(L.SITEBOND, b1, b2, socc, bocc, canon, 1)
    assert (got == pairs_mask(b1, b2, col)).all()
    with pytest.raises(ValueError):
        api.conducting_bonds(L.BONDSITE, b1, b2, socc, bocc, canon, 1)


def test_errors_are_einval():
    lib = L.lib()
    lat = (0, 10, 10, 0)
    nb = api.nbonds(*lat)
    mask, v = np.ones(nb, np.uint8), np.zeros(80)
    rec = np.zeros(1, dtype=L.CURRENTS_DTYPE)

    def call(lattice=0, m=10, n=10, pbc=0, mask=mask, v=v, cut=CUT, out=rec):
        return lib.perc_current_stats_host(lattice, m, n, pbc, L.ptr(mask), L.ptr(v), 1.0, 1.0, cut, L.ptr(out))

    assert call() == L.PERC_OK
    for kw in (dict(lattice=2), dict(lattice=-1), dict(m=0), dict(n=0), dict(mask=None), dict(v=None),
               dict(out=None), dict(cut=-1e-9), dict(cut=1.0 + 1e-9), dict(cut=float("nan"))):
        assert call(**kw) == -1, kw
        assert lib.perc_last_error().decode().startswith("perc_current_stats_host:"), kw
    for cut in (-0.5, 2.0, float("nan")):
        with pytest.raises(L.PercError, match="PERC_EINVAL"):
            api.current_stats_host(*lat, mask, v, cut=cut)
    with pytest.raises(ValueError):
        api.current_stats_host(*lat, mask[:-1], v)
    with pytest.raises(ValueError):
        api.current_stats_host(*lat, mask, v[:-1])
    # a NULL context: PERC_EINVAL before anything else
    for name in ("perc_batch_cond_currents", "perc_batch_cond_currents_seeded"):
        assert getattr(lib, name)(None, L.BOND, L.RULE_BOND, L.CUR_FORTRAN, 0, None, None, 0, None, None, None,
                                  1.0, 1.0, 1e-12, 2, 1e-8, 2500, None, CUT, None, None) == -1


def test_abi():
    """the entry points are in the library, in SIGNATURES, in the header and
    in the Fortran module; the record is 304 bytes; the predicate is exactly
    perc_batch_cond_supported"""
    lib = L.lib()
    header = open(os.path.join(REPO, "include", "perc.h")).read()
    f90 = open(os.path.join(REPO, "percolation_amd", "fortran", "perc_mod.f90")).read()
    for name in ("perc_batch_currents_supported", "perc_batch_cond_currents", "perc_batch_cond_currents_seeded",
                 "perc_current_stats_host"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
        assert name + "(" in header and "name='%s'" % name in f90, name
    assert L.SIGNATURES["perc_batch_cond_currents"][1] == L.SIGNATURES["perc_batch_cond_currents_seeded"][1]
    # perc_batch_cond's arguments without solve, then cut, cur, vint_out
    a, b = L.SIGNATURES["perc_batch_cond_currents"][1], L.SIGNATURES["perc_batch_cond"][1]
    assert a[:11] == b[:11] and a[11:18] == b[12:] and len(a) == len(b) - 1 + 3
    assert L.CURRENTS_DTYPE.itemsize == 304 and L.CURRENTS_DTYPE.fields["hist"][1] == 48
    for kind in (L.BOND, L.SITE, L.SITEBOND, L.BONDSITE):
        for lat in LATTICES + [(0, 64, 130, 0), (0, 91, 93, 0), (0, 128, 128, 0), (1, 11, 10, 0), (0, 2, 10, 0)]:
            assert api.batch_currents_supported(kind, *lat) == api.batch_cond_supported(kind, *lat), (kind, lat)
    assert api.batch_currents_supported(L.BOND, 0, 64, 130, 0) and not api.batch_currents_supported(L.BOND, 0, 91, 93, 0)
