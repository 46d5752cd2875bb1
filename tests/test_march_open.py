"""The open-lattice instantiation of the strip-major nibble march.

On an open lattice the strip-major nibble kernels (the metric's P and B) run
an instantiation of k_cg_march that holds the open-square path alone: no form
test, no run-time-mask, map or general path and none of their LDS tables.
Under pbc the strip-major nibble march keeps the other instantiation, which
no longer holds the open-square path.  Every row's arithmetic and every sum's
association must stay what they were.

Shapes: the smallest at which the walk can go wrong (m a multiple of 128 and
N > 8192, so the march runs): 128 x 300, one strip with both edge-column
spreads in one wave; 384 x 40, an interior strip between two edge strips.
Band heights (set_march_rows): every height from 1 to 2 D + 3 = 9 (D = 3 rows
prefetched) -- bands shorter than, equal to and up to three times the
prefetch ring, with 0, 1 and 2 steps of the last group of D past the walk --,
43 (the metric's height) on the 300-row case and the automatic height.  Every
case has at least two bands per strip and alternating walk directions, so
both directions run.

* literal dot order against the oracle's literal linbcg (test_march_cmask.py's
  protocol): iter, the whole err history, Gtop, Gbot and every voltage
  bitwise, at tol 1e-8 and 1e-13;
* fast order against the same context with PERC_MARCH_NIBBLE off: the u16
  kernels are untouched by the change;
* selection: last_solve()["open"] is true on the open cases, false under pbc
  (strip-major, nibble codes kept) and false for the row-major march.
"""
import numpy as np
import pytest

import oracle_lib as O
from percolation_amd import _lib as PL
from percolation_amd import api

pytestmark = pytest.mark.gpu

MARCH_ONLY = PL.MARCH_DEFAULT & ~PL.SOLVE_RESIDENT
MARCH_ROWMAJOR = MARCH_ONLY & ~PL.MARCH_STRIPS
DEPTH = 3  # rows the strip-major march prefetches (k_cg_march's D)

# (lattice, m, n, pbc, p, seed): oracle iterations at tol 1e-8
OPEN = [
    (0, 128, 300, 0, 0.62, 43),   # 1610: one strip, tall
    (0, 384, 40, 0, 0.60, 42),    # 563: three strips
]
PBC = (0, 256, 67, 1, 0.60, 44)   # 759
TOLS = (1e-8, 1e-13)

_SYSTEM = {}
_ORACLE = {}


def system(case):
    """the case's occupation and bond values (computed once per case)"""
    if case not in _SYSTEM:
        lat, m, n, pbc, p, seed = case
        b1, b2 = api.bond_list(lat, m, n, pbc)
        nb = len(b1)
        order = api.shuffled_ids(nb, seed)
        tb = int(p * nb)
        ref = api.replay_labels(lat, m, n, pbc, PL.BOND, bond_order=order, nbond=tb)
        assert ref["perccln"] > 0, case
        gval = O.f64(nb)
        O.lib().or_bond_values(0, nb, b1, b2, ref["bond_label"], O.i32(1), ref["perccln"], 1.0, 1e-12, gval)
        _SYSTEM[case] = (b1, b2, gval, order, tb)
    return _SYSTEM[case]


def oracle(case, tol):
    """the oracle's literal linbcg of the case (computed once per case and tol)"""
    if (case, tol) not in _ORACLE:
        lat, m, n, pbc, _, _ = case
        b1, b2, gval, _, _ = system(case)
        _ORACLE[(case, tol)] = O.conductance(lat, m, n, pbc, b1, b2, gval, tol=tol, itmax=100000)
    return _ORACLE[(case, tol)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def band_rows(case):
    rows = [0] + list(range(1, 2 * DEPTH + 4))
    return rows + [43] if case[2] == 300 else rows


CASE_ROWS = [(c, r) for c in OPEN for r in band_rows(c)]
IDS = ["%dx%d-rows%d" % (c[1], c[2], r) for c, r in CASE_ROWS]


def check_bands(ctx, case, rows):
    """static bands of the requested height, at least two per strip, walking
    in alternating directions"""
    info = ctx.march_info()
    assert info["alt"] and not info["slots"], info
    if rows:
        assert info["band_rows"] == rows, info
    assert 2 * info["band_rows"] <= case[2] - 2, info


@pytest.mark.parametrize("case,rows", CASE_ROWS, ids=IDS)
def test_literal_open_march_is_the_oracle_linbcg_bitwise(case, rows):
    lat, m, n, pbc, _, _ = case
    _, _, _, order, tb = system(case)
    with api.Context(lat, m, n, pbc) as ctx:
        ctx.set_march_mode(MARCH_ONLY)
        ctx.set_dot_order(PL.DOT_LITERAL)
        ctx.set_march_rows(rows)
        ctx.occupy(PL.BOND, bond_order=order, nbonds_=tb)
        assert ctx.label()["nspan"] > 0
        for tol in TOLS:
            oc = oracle(case, tol)
            c = ctx.conductance(tol=tol, itmax=100000, vint=True)
            hist = ctx.err_history()
            ran = ctx.last_solve()
            check_bands(ctx, case, rows)
            assert ran["kernel"] == "march" and ran["literal"] and ran["lit_terms"], ran
            assert ran["qfree"] and ran["strips"] and ran["nibble"] and ran["open"], ran
            assert ran["iter"] == c["iter"], ran
            assert c["iter"] == oc["iter"], (tol, c["iter"], oc["iter"])
            assert np.array_equal(bits(hist), bits(oc["errs"])), tol
            assert c["gtop"] == oc["gtop"] and c["gbot"] == oc["gbot"], (tol, c["gtop"], oc["gtop"])
            assert np.array_equal(bits(c["vint"]), bits(oc["vint"])), tol


@pytest.mark.parametrize("case,rows", CASE_ROWS, ids=IDS)
def test_fast_open_march_is_the_u16_march_bitwise(case, rows):
    """the whole fast-order solve on the open-lattice nibble kernels against
    the u16 kernels of the same context"""
    lat, m, n, pbc, _, _ = case
    _, _, _, order, tb = system(case)
    with api.Context(lat, m, n, pbc) as ctx:
        ctx.set_march_rows(rows)
        ctx.occupy(PL.BOND, bond_order=order, nbonds_=tb)
        assert ctx.label()["nspan"] > 0
        for tol in TOLS:
            out = []
            for mode in (MARCH_ONLY, MARCH_ONLY & ~PL.MARCH_NIBBLE):
                ctx.set_march_mode(mode)
                c = ctx.conductance(tol=tol, itmax=100000, vint=True)
                c["hist"] = ctx.err_history()
                ran = ctx.last_solve()
                check_bands(ctx, case, rows)
                assert ran["kernel"] == "march" and ran["qfree"] and ran["strips"], ran
                nib = bool(mode & PL.MARCH_NIBBLE)
                assert ran["nibble"] == nib and ran["open"] == nib, ran
                out.append(c)
            a, b = out
            assert a["iter"] == b["iter"] and a["iter"] > 100, (tol, a["iter"], b["iter"])
            assert np.array_equal(bits(a["hist"]), bits(b["hist"])), tol
            assert a["gtop"] == b["gtop"] and a["gbot"] == b["gbot"], tol
            assert np.array_equal(bits(a["vint"]), bits(b["vint"])), tol


def test_pbc_strip_major_march_is_not_open():
    """under pbc the strip-major march keeps its nibble codes and the
    instantiation with the run-time-mask, map and general paths"""
    lat, m, n, pbc, _, _ = PBC
    _, _, _, order, tb = system(PBC)
    with api.Context(lat, m, n, pbc) as ctx:
        ctx.set_march_mode(MARCH_ONLY)
        ctx.occupy(PL.BOND, bond_order=order, nbonds_=tb)
        assert ctx.label()["nspan"] > 0
        c = ctx.conductance(tol=1e-8, itmax=100000)
        ran = ctx.last_solve()
        assert ran["kernel"] == "march" and ran["qfree"] and ran["strips"] and ran["iter"] == c["iter"], ran
        assert ran["nibble"] and not ran["open"], ran


def test_row_major_march_is_not_open():
    case = OPEN[1]
    lat, m, n, pbc, _, _ = case
    _, _, _, order, tb = system(case)
    with api.Context(lat, m, n, pbc) as ctx:
        ctx.set_march_mode(MARCH_ROWMAJOR)
        ctx.occupy(PL.BOND, bond_order=order, nbonds_=tb)
        assert ctx.label()["nspan"] > 0
        c = ctx.conductance(tol=1e-8, itmax=100000)
        ran = ctx.last_solve()
        assert ran["kernel"] == "march" and ran["qfree"] and not ran["strips"] and ran["iter"] == c["iter"], ran
        assert ran["nibble"] and not ran["open"], ran
