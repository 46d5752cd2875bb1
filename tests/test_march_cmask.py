"""The march's open-square stencil built from a compile-time position mask.

The nibble-code instantiations of k_cg_march (strip-major: the metric's
kernels; row-major: the L > 4096 companion's) form a row's four neighbour
terms from kSqRasterMask at compile time instead of evaluating all eight
raster positions under the forms table's run-time mask.  The sum must stay
bitwise what it was: the same terms in the same slot order.

Checked two ways on the smallest shapes at which the walk can still go
wrong (m a multiple of 128 and N > 8192, so the march runs and not the
one-workgroup solver; one strip -- both edge-column spreads in one wave;
three and five strips -- interior strips between two edge strips; bands
shorter than the prefetch ring; pbc and triangular lattices, which must not
take the new path):

* literal dot order against the oracle's literal linbcg (test_literal_dot.py's
  protocol): iter, the whole err history, Gtop, Gbot and every voltage
  bitwise, at tol 1e-8 and 1e-13, through the strip-major and the row-major
  march, with automatic bands and with set_march_rows(7) (bands of several
  rows and a remainder; 43, the metric's band height, on the 300-row case);
* fast order against the same context with PERC_MARCH_NIBBLE off: the u16
  kernels keep the run-time mask and are untouched by the change.

The open square cases must have run nibble codes.  The triangular lattice
and the row-major march under pbc must not have.  The strip-major march
under pbc keeps its nibble codes (test_gpu_parity.py's
test_nibble_codes_are_bitwise_the_u16_codes pins that): its kernel takes the
run-time-mask paths there (march_step: sqp = !pbc), which the bitwise
comparison with the oracle covers.
"""
import numpy as np
import pytest

import oracle_lib as O
from percolation_amd import _lib as PL
from percolation_amd import api

pytestmark = pytest.mark.gpu

MARCH_ONLY = PL.MARCH_DEFAULT & ~PL.SOLVE_RESIDENT
MARCH_ROWMAJOR = MARCH_ONLY & ~PL.MARCH_STRIPS

# (lattice, m, n, pbc, p, seed): oracle iterations at tol 1e-8
CASES = [
    (0, 128, 70, 0, 0.60, 41),    # 700: one strip
    (0, 384, 40, 0, 0.60, 42),    # 563: three strips
    (0, 128, 300, 0, 0.62, 43),   # 1610: one strip, tall
    (0, 640, 24, 0, 0.60, 46),    # 357: five strips, bands shorter than the prefetch ring
    (0, 256, 67, 1, 0.60, 44),    # 759: pbc
    (1, 128, 80, 0, 0.42, 45),    # 764: triangular
]
OPEN_SQUARE = [c for c in CASES if c[0] == 0 and not c[3]]
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


def nibble_expected(case, strips):
    lat, _, _, pbc, _, _ = case
    return lat == 0 and (not pbc or strips)


def band_rows(case):
    return (0, 7, 43) if case[2] == 300 else (0, 7)


LITERAL = [(c, s, r) for c in CASES for s in (True, False) for r in band_rows(c)]


@pytest.mark.parametrize("case,strips,rows", LITERAL,
                         ids=["%d-%dx%d-pbc%d-%s-rows%d" % (c[0], c[1], c[2], c[3], "sm" if s else "rm", r)
                              for c, s, r in LITERAL])
def test_literal_march_is_the_oracle_linbcg_bitwise(case, strips, rows):
    lat, m, n, pbc, _, _ = case
    _, _, _, order, tb = system(case)
    with api.Context(lat, m, n, pbc) as ctx:
        if strips:
            ctx.set_march_mode(MARCH_ONLY)
            ctx.set_dot_order(PL.DOT_LITERAL)
        else:
            ctx.set_march_mode(MARCH_ROWMAJOR)
            ctx.set_dot_order(PL.DOT_LITERAL_HOST)
        ctx.set_march_rows(rows)
        ctx.occupy(PL.BOND, bond_order=order, nbonds_=tb)
        assert ctx.label()["nspan"] > 0
        for tol in TOLS:
            oc = oracle(case, tol)
            c = ctx.conductance(tol=tol, itmax=100000, vint=True)
            hist = ctx.err_history()
            ran = ctx.last_solve()
            assert ran["kernel"] == "march" and ran["literal"] and ran["lit_terms"], ran
            assert ran["qfree"] and ran["strips"] == strips and ran["iter"] == c["iter"], ran
            assert ran["nibble"] == nibble_expected(case, strips), ran
            assert c["iter"] == oc["iter"], (tol, c["iter"], oc["iter"])
            assert np.array_equal(bits(hist), bits(oc["errs"])), tol
            assert c["gtop"] == oc["gtop"] and c["gbot"] == oc["gbot"], (tol, c["gtop"], oc["gtop"])
            assert np.array_equal(bits(c["vint"]), bits(oc["vint"])), tol


@pytest.mark.parametrize("strips", [True, False], ids=["sm", "rm"])
@pytest.mark.parametrize("case", OPEN_SQUARE, ids=["%dx%d" % (c[1], c[2]) for c in OPEN_SQUARE])
def test_fast_march_is_the_u16_march_bitwise(case, strips):
    """the whole fast-order solve on nibble codes (compile-time mask) against
    the u16 codes (run-time mask) of the same context"""
    lat, m, n, pbc, _, _ = case
    _, _, _, order, tb = system(case)
    base = MARCH_ONLY if strips else MARCH_ROWMAJOR
    with api.Context(lat, m, n, pbc) as ctx:
        ctx.occupy(PL.BOND, bond_order=order, nbonds_=tb)
        assert ctx.label()["nspan"] > 0
        for tol in TOLS:
            out = []
            for mode in (base, base & ~PL.MARCH_NIBBLE):
                ctx.set_march_mode(mode)
                c = ctx.conductance(tol=tol, itmax=100000, vint=True)
                c["hist"] = ctx.err_history()
                ran = ctx.last_solve()
                assert ran["kernel"] == "march" and ran["qfree"] and ran["strips"] == strips, ran
                assert ran["nibble"] == bool(mode & PL.MARCH_NIBBLE), ran
                out.append(c)
            a, b = out
            assert a["iter"] == b["iter"] and a["iter"] > 100, (tol, a["iter"], b["iter"])
            assert np.array_equal(bits(a["hist"]), bits(b["hist"])), tol
            assert a["gtop"] == b["gtop"] and a["gbot"] == b["gbot"], tol
            assert np.array_equal(bits(a["vint"]), bits(b["vint"])), tol
