"""Site and mixed rules, pbc, both lattices and non-unit Va / g0 / leak on
every solver path, against the oracle (oracle/perc_oracle.c: or_bond_values,
or_assemble, the literal linbcg, or_currents).

The rest of the suite pins the bond rule at Va = g0 = 1, leak = 1e-12, where
every product g0 * x and gval * Va is exact and the 1e-12 leak terms are
always dropped by the Fortran-rule current threshold (|g| >= 1e-10,
bondc.f:547): a kernel that hard-codes a value, scales the right-hand side by
the wrong one, swaps -g0 and -leak or keeps the wrong current terms passes
there.  Here the 36 systems of rule_systems.matrix() run

* assembled (CSR arrays, diagonal, rhs) and multiplied (SpMV) bitwise the
  oracle's, in the four explicit formats;
* solved in the literal dot order through every solver family -- the
  one-workgroup solve, the resident solve, the strip-major and the row-major
  march, the LDS-tiled, split and CSR launched kernels -- bitwise the oracle's
  linbcg at tol 1e-8 and 1e-13: iteration count, err history, every voltage,
  and Gtop / Gbot under both current rules (bondc.f's with its 1e-10
  threshold, ConductCalc.m's without one);
* solved in the default (fast) order, single and in 3 row slabs, to the
  project's existing bars: test_config_goldens.py's at tol 1e-8 (iterations
  +-1, G within 2 trunc + max(1e-10, tol), trunc the oracle's own relative move
  from 1e-8 to 1e-13) and SURVEY.md §8(c)'s 1e-10 at tol 1e-13.  The flat bars
  need no widening here: the oracle re-run with its sums reversed
  (conductance_decades, dot_order 1) moves G by at most 2.3e-9 at 1e-8 and
  3.7e-13 at 1e-13 on these systems;
* with ConductCalc.m's per-bond weights on the launched CSR kernels (N > 8192).

Every solve asserts which kernel family ran (perc_last_solve,
perc_matrix_format): a silent fallback fails.  The CPU tests check that the
systems span, that the oracle's solves stop by tolerance, that the value sets
straddle the current threshold, and that the family x rule x value grid is
covered.
"""
import numpy as np
import pytest

import oracle_lib as O
import rule_systems as R
from percolation_amd import _lib as PL
from percolation_amd import api

REL = 1e-10
MATRIX = R.matrix()
FORMATS = [PL.FMT_STENCIL, PL.FMT_STENCIL_TILED, PL.FMT_STENCIL_SPLIT, PL.FMT_CSR]
MARCH_ONLY = PL.MARCH_DEFAULT & ~PL.SOLVE_RESIDENT
MARCH_ROWMAJOR = MARCH_ONLY & ~PL.MARCH_STRIPS

# the solver families a geometry reaches (perc_solve.hip: select_format,
# res_geometry).  resident / small / "march" under pbc: PERC_FMT_AUTO; the
# open lattices' march: PERC_SOLVE_RESIDENT cleared; tiled / split / csr: the
# explicit format (PERC_FMT_STENCIL on m = 130 would run the resident solve,
# which select_format prefers whenever its grid exists: PERC_FMT_STENCIL_TILED
# asks for the tiles themselves)
FAMILIES = ("small", "resident", "march", "march_rowmajor", "tiled", "split", "csr")
LAUNCHED = ("tiled", "split", "csr")
SOLVERS = {
    R.G_OPEN_SQ: ("resident", "march", "march_rowmajor") + LAUNCHED,
    R.G_OPEN_TRI: ("resident", "march", "march_rowmajor") + LAUNCHED,
    # wrapped forms: no resident grid, PERC_FMT_AUTO runs the march
    R.G_PBC_SQ: ("march", "march_rowmajor") + LAUNCHED,
    R.G_PBC_TRI: ("march", "march_rowmajor") + LAUNCHED,
    R.G_TILE_SQ: ("resident",) + LAUNCHED,
    R.G_TILE_TRI: LAUNCHED,
    R.G_SMALL_SQ: ("small", "split", "csr"),
    R.G_SMALL_TRI: ("small", "split", "csr"),
}
LITERAL_CASES = [(s, f) for s in MATRIX for f in SOLVERS[R.geometry(s)]]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def sid(s):
    return R.name(s)


# ------------------------------------------------------------ CPU
@pytest.mark.parametrize("s", MATRIX, ids=sid)
def test_system_spans_and_oracle_stops_by_tolerance(s):
    """every system of the matrix spans with one spanning label, and the
    oracle's linbcg stops by the tolerance (not by itmax) at 1e-8 and 1e-13"""
    d = R.build(s)
    assert d["perccln"] > 0 and d["nspan"] == 1, (d["perccln"], d["nspan"])
    inc = d["gval"] == -s.g0
    assert inc.any() and (d["gval"][~inc] == -s.leak).all()
    for tol in R.TOLS:
        oc = R.oracle_solve(s, tol)
        assert 0 < oc["iter"] < R.ITMAX and oc["err"] <= tol, (tol, oc["iter"], oc["err"])
        assert oc["cur"][PL.CUR_FORTRAN][0] > 0 and oc["cur"][PL.CUR_MATLAB][0] > 0


def test_matrix_is_the_stated_one():
    assert len(MATRIX) == len(set(MATRIX)) == 36
    for rule in (PL.RULE_SITE, PL.RULE_MIXED):
        mine = [s for s in MATRIX if s.rule == rule]
        assert {R.geometry(s) for s in mine if not R.nonunit(s)} == set(R.GEOMETRIES)
        assert {(R.geometry(s), s[5:]) for s in mine if R.nonunit(s)} == {(R.G_OPEN_SQ, v) for v in R.NONUNIT}
    bond = [s for s in MATRIX if s.rule == PL.RULE_BOND]
    assert {(R.geometry(s), s[5:]) for s in bond} == {(g, v) for g in R.GEOMETRIES for v in R.NONUNIT}


@pytest.mark.parametrize("s", [s for s in MATRIX if R.nonunit(s)], ids=sid)
def test_value_sets_straddle_the_current_threshold(s):
    """leak = 3e-11 < 1e-10: the Fortran rule drops the leak terms that the
    MATLAB rule keeps, and Gtop shows it (> 1e-9 relative); leak = 3e-9: both
    keep every term and differ by the order of the sum only (< 1e-12)"""
    for tol in R.TOLS:
        cur = R.oracle_solve(s, tol)["cur"]
        d = rel(cur[PL.CUR_FORTRAN][0], cur[PL.CUR_MATLAB][0])
        print("%s tol %g: Gtop Fortran rule vs MATLAB rule %.3e" % (R.name(s), tol, d))
        if s.leak < R.CUR_THRESH[PL.CUR_FORTRAN]:
            assert d > 1e-9, (tol, d)
        else:
            assert d < 1e-12, (tol, d)


def test_conductance_scales_with_g0():
    """G is linear in g0 up to the leak's share: G(g0 = 0.7) / G(g0 = 1) is
    0.7 to 1e-6 (bond rule; Va cancels in G = I / Va)"""
    a = R.System(PL.RULE_BOND, *R.G_OPEN_SQ, *R.LEAK_DROPPED)
    b = R.System(PL.RULE_BOND, *R.G_OPEN_SQ, *R.UNIT)
    ga, gb = R.oracle_solve(a, 1e-13)["gtop"], R.oracle_solve(b, 1e-13)["gtop"]
    assert abs(ga / gb - a.g0) < 1e-6, (ga, gb, ga / gb)


def test_literal_cases_cover_family_rule_value_grid():
    """every solver family is reached by a site system, a mixed system and a
    non-unit system; both lattices and both pbc settings occur for each rule"""
    for fam in FAMILIES:
        mine = [s for s, f in LITERAL_CASES if f == fam]
        assert any(s.rule == PL.RULE_SITE for s in mine), fam
        assert any(s.rule == PL.RULE_MIXED for s in mine), fam
        assert any(R.nonunit(s) for s in mine), fam
    assert {f for _, f in LITERAL_CASES} == set(FAMILIES)
    for rule in R.RULE_NAME:
        mine = [s for s in MATRIX if s.rule == rule]
        assert {(s.lattice, s.pbc) for s in mine} == {(0, 0), (0, 1), (1, 0), (1, 1)}, rule
    assert set(SOLVERS) == set(R.GEOMETRIES)


# ------------------------------------------------------------ GPU
def used_fmt(fmt, m):
    """perc_matrix_format's answer to a request: PERC_FMT_STENCIL is the
    register march when m is a multiple of 128, else the LDS tiles"""
    return PL.FMT_STENCIL_TILED if fmt == PL.FMT_STENCIL and m % 128 else fmt


def occupied(s, d):
    """a labeled context of the system; its spanning test agrees with the oracle's"""
    ctx = api.Context(*R.geometry(s))
    try:
        ctx.occupy(**d["occ"])
        assert ctx.label()["nspan"] == d["nspan"] == 1
    except BaseException:
        ctx.close()
        raise
    return ctx


@pytest.mark.gpu
@pytest.mark.parametrize("s", MATRIX, ids=sid)
def test_assembly_and_spmv_bitwise(s):
    """perc_get_system's CSR arrays, diagonal and rhs are or_assemble's on the
    rule's bond values with the system's Va, and the SpMV is or_dsprsax's,
    bitwise, in every explicit format"""
    d = R.build(s)
    oc = R.oracle_solve(s, 1e-8)  # (its assembled system: sa, ija, itemp)
    sa, ija, itemp, k = oc["sa"], oc["ija"], oc["itemp"], oc["nnz"]
    N = s.m * s.n - 2 * s.m
    x = np.random.default_rng(s.m * 1000 + s.n).standard_normal(N)
    yo = O.f64(N)
    O.lib().or_dsprsax(sa, ija, x, yo, N)
    with occupied(s, d) as ctx:
        for fmt in FORMATS:
            ctx.set_matrix_format(fmt)
            ctx.conductance(s.rule, R.natural_cur_rule(s), s.Va, s.g0, s.leak, itmax=3)
            assert ctx.matrix_format() == used_fmt(fmt, s.m), fmt
            sysm = ctx.system()
            # NR layout -> CSR
            assert np.array_equal(sysm["rowptr"], ija[:N + 1] - (N + 2)), fmt
            assert np.array_equal(sysm["col"], ija[N + 1:k] - 1), fmt
            assert np.array_equal(bits(sysm["val"]), bits(sa[N + 1:k])), fmt
            assert np.array_equal(bits(sysm["diag"]), bits(sa[:N])), fmt
            assert np.array_equal(bits(sysm["rhs"]), bits(itemp)), fmt
            assert np.array_equal(bits(ctx.spmv(x)), bits(yo)), fmt


def select(ctx, family):
    """ask for a solver family; literal: the dot order that family folds in"""
    order = PL.DOT_LITERAL
    if family == "march":
        if not ctx.pbc:
            ctx.set_march_mode(MARCH_ONLY)
    elif family == "march_rowmajor":
        # (the row-major march's sums are folded by the host)
        ctx.set_march_mode(MARCH_ROWMAJOR)
        order = PL.DOT_LITERAL_HOST
    elif family in LAUNCHED:
        ctx.set_matrix_format({"tiled": PL.FMT_STENCIL_TILED, "split": PL.FMT_STENCIL_SPLIT,
                               "csr": PL.FMT_CSR}[family])
    return order


def check_family(ctx, family, literal):
    """the kernel family the last solve ran is the one asked for"""
    ran, fmt = ctx.last_solve(), ctx.matrix_format()
    lat, m, pbc = ctx.lattice, ctx.m, ctx.pbc
    assert ran["literal"] == literal, ran
    if family == "small":
        assert ran["kernel"] == "small", ran
    elif family == "resident":
        assert ran["kernel"] == "resident" and ran["lit_terms"] == literal, ran
        assert fmt == (PL.FMT_STENCIL if m % 128 == 0 else PL.FMT_STENCIL_TILED), fmt
    elif family == "march":
        # the strip-major q-free march, tagged reductions; nibble codes on the
        # open square lattice
        assert ran["kernel"] == "march" and ran["lit_terms"] == literal and fmt == PL.FMT_STENCIL, (ran, fmt)
        assert ran["qfree"] and ran["strips"] and ran["tag"] and not ran["host_fold"], ran
        assert ran["nibble"] or lat != 0 or pbc, ran
    elif family == "march_rowmajor":
        assert ran["kernel"] == "march" and ran["lit_terms"] and ran["host_fold"], ran
        assert ran["qfree"] and not ran["strips"] and fmt == PL.FMT_STENCIL, (ran, fmt)
        assert ran["nibble"] or lat != 0 or pbc, ran
    else:
        want = {"tiled": PL.FMT_STENCIL_TILED, "split": PL.FMT_STENCIL_SPLIT, "csr": PL.FMT_CSR}[family]
        assert ran["kernel"] == "other" and not ran["lit_terms"] and fmt == want, (ran, fmt)


def literal_solves(ctx, s, family, tol, oc):
    """the system solved in the literal order under both current rules (the
    rule's own with every voltage returned; the other with x carried on the
    electrode-side rows only, the default) against the oracle's oc, bitwise"""
    own = R.natural_cur_rule(s)
    other = PL.CUR_MATLAB if own == PL.CUR_FORTRAN else PL.CUR_FORTRAN
    for cur in (own, other):
        c = ctx.conductance(s.rule, cur, s.Va, s.g0, s.leak, tol=tol, itmax=R.ITMAX, vint=cur == own)
        check_family(ctx, family, True)
        assert c["iter"] == oc["iter"], (tol, cur, c["iter"], oc["iter"])
        assert np.array_equal(bits(ctx.err_history()), bits(oc["errs"])), (tol, cur)
        assert (c["gtop"], c["gbot"]) == oc["cur"][cur], (tol, cur, c["gtop"], c["gbot"], oc["cur"][cur])
        if cur == own:
            assert np.array_equal(bits(c["vint"]), bits(oc["vint"])), tol


@pytest.mark.gpu
@pytest.mark.parametrize("s,family", LITERAL_CASES, ids=lambda v: v if isinstance(v, str) else sid(v))
def test_literal_solve_is_the_oracle_linbcg_bitwise(s, family):
    d = R.build(s)
    with occupied(s, d) as ctx:
        ctx.set_dot_order(select(ctx, family))
        for tol in R.TOLS:
            literal_solves(ctx, s, family, tol, R.oracle_solve(s, tol))


def default_family(s):
    return SOLVERS[R.geometry(s)][0]


@pytest.mark.gpu
@pytest.mark.parametrize("s", MATRIX, ids=sid)
def test_fast_order_meets_the_existing_bars(s):
    """the default path (PERC_FMT_AUTO, the fast dot order) and, where the
    register march exists (m % 128 == 0), 3 row slabs"""
    d = R.build(s)
    o8, o13 = R.oracle_solve(s, 1e-8), R.oracle_solve(s, 1e-13)
    cur = R.natural_cur_rule(s)
    runs = [("default", 1)] + ([("slabs", 3)] if s.m % 128 == 0 else [])
    with occupied(s, d) as ctx:
        for what, nslab in runs:
            ctx.set_slabs(nslab)
            c8 = ctx.conductance(s.rule, cur, s.Va, s.g0, s.leak, tol=1e-8, itmax=R.ITMAX)
            if nslab == 1:
                check_family(ctx, default_family(s), False)
            else:
                assert ctx.last_solve()["kernel"] == "slabs" and ctx.matrix_format() == PL.FMT_STENCIL
            c13 = ctx.conductance(s.rule, cur, s.Va, s.g0, s.leak, tol=1e-13, itmax=R.ITMAX)
            dist = {}
            for i, g in enumerate(("gtop", "gbot")):
                trunc = rel(o8["cur"][cur][i], o13["cur"][cur][i])
                dist[g] = (rel(c8[g], o8["cur"][cur][i]), 2 * trunc + max(1e-10, 1e-8),
                           rel(c13[g], o13["cur"][cur][i]))
            print("%s %s: iter %d (oracle %d); 1e-8: Gtop %.3e Gbot %.3e; 1e-13: Gtop %.3e Gbot %.3e"
                  % (R.name(s), what, c8["iter"], o8["iter"], dist["gtop"][0], dist["gbot"][0],
                     dist["gtop"][2], dist["gbot"][2]))
            assert abs(c8["iter"] - o8["iter"]) <= 1, (what, c8["iter"], o8["iter"])
            for g, (d8, bar8, d13) in dist.items():
                assert d8 <= bar8, (what, g, d8, bar8)
                assert d13 < REL, (what, g, d13)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", sorted(R.RULE_NAME), ids=lambda r: R.RULE_NAME[r])
def test_conductcalc_weights_on_launched_csr_bitwise(rule):
    """ConductCalc.m condtype 2 at N = 12416 > 8192 (the launched CSR kernels,
    not k_cg_small): the weights perc_set_conductcalc_weights draws, in the
    literal order, against the oracle on gval = -g0 * w for the rule's bonds"""
    s = R.System(rule, *R.G_OPEN_SQ, *R.LEAK_DROPPED)
    d = R.build(s)
    assert d["perccln"] > 0
    w = api.conductcalc_weights(rule, d["b1"], d["b2"], d["blabel"],
                                d["slabel"] if rule != PL.RULE_BOND else None, d["perccln"])
    gval = d["gval"].copy()
    inc = gval == -s.g0
    assert inc.sum() > 1000 and (w[~inc] == 1.0).all() and (w[inc] < 1.0).all()
    gval[inc] = -s.g0 * w[inc]
    with occupied(s, d) as ctx:
        ctx.set_dot_order(PL.DOT_LITERAL)
        ctx.set_conductcalc_weights(rule)
        for tol in R.TOLS:
            oc = R.oracle_conductance(s, d, tol, gval)
            assert oc["iter"] < R.ITMAX and oc["err"] <= tol
            literal_solves(ctx, s, "csr", tol, oc)
