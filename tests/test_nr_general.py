"""The NR drop-in on the device, on matrices the lattice never produces.

libperc's dsprsax_, dsprstx_, atimes_ and linbcg_ (perc_nr.cpp, ctypes) take
any matrix in NR row-indexed storage.  The matrices of nr_systems.py reach
what the lattice systems of test_nr_symbols.py / test_itol.py cannot: rows
of 0 .. 11 off-diagonals (k_spmv<4>, <6> and the looped <0>, k_cg_spmv_row
likewise), rows without entries (also at the very end of the storage), sizes
around the workgroup and reduction-group boundaries, non-symmetric matrices
(the explicit transpose of spmv_nr), a symmetric pattern with one value an
ulp off, non-zero starts (r = b - A x in k_cg_init / k_x34_init), itol 1,
the fast dot order, the itmax edges and one device context reused over
matrices of changing N and entry count.

The reference is the oracle's literal restatement of the same routine
(or_dsprsax, or_dsprstx, or_linbcg; checked against a dense product in
test_nr_general_host.py).  Products and the literal solve are compared
bitwise; the fast order against the oracle's own re-association spread
(max(1e-10, 1.5 x the spread)).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import nr_systems as S
import oracle_lib as O
import percolation_amd as P

pytestmark = pytest.mark.gpu

DOT_FAST, DOT_LITERAL = 0, 1
TOL, ITMAX = 1e-10, 5000

SPMV_N = (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 513, 1500, 16385, 20001)
SOLVE = [(1, 0), (2, 1), (3, 2), (65, 4), (257, 6), (513, 11), (1500, 4), (1500, 11), (16385, 6),
         (20001, 11)]
SOLVE34 = [(257, 6), (1500, 11)]
STARTS = ("zero", "normal")
LITERAL_CASES = [(n, mr, itol) for n, mr in SOLVE for itol in (1, 2)] + \
                [(n, mr, itol) for n, mr in SOLVE34 for itol in (3, 4)]
FAST_CASES = [(n, mr, itol) for n, mr in SOLVE for itol in (1, 2)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def sym(n, maxrow, seed=None):
    rows, diag = S.sym_spd(n, maxrow, S.seed_of(n, maxrow) if seed is None else seed,
                           empty=S.edge_rows(n))
    sa, ija = S.to_nr(rows, diag)
    cnt = max(len(c) for c, _ in rows)
    assert cnt == maxrow or n < 63  # the row-length class the case is for
    sa.setflags(write=False)
    ija.setflags(write=False)
    return sa, ija


@functools.lru_cache(maxsize=None)
def gen(n, maxrow):
    rows, diag = S.general(n, maxrow, S.seed_of(n, maxrow))
    sa, ija = S.to_nr(rows, diag)
    sa.setflags(write=False)
    ija.setflags(write=False)
    return sa, ija


def start(n, which):
    return np.zeros(n) if which == "zero" else S.xvec(n, salt=1)


@functools.lru_cache(maxsize=None)
def ref_solve(n, maxrow, itol, which, tol=TOL, itmax=ITMAX, seed=None):
    """the oracle's literal linbcg: (x, iter, err)"""
    sa, ija = sym(n, maxrow, seed)
    x, it, err = O.nr_linbcg(sa, ija, S.bvec(n), start(n, which), itol, tol, itmax)
    x.setflags(write=False)
    return x, it, err


@functools.lru_cache(maxsize=None)
def ref_spread(n, maxrow, K):
    """the oracle's own association spread of x after K iterations from x =
    0: dot products summed descending against ascending, max |dx| / max |x|"""
    sa, ija = sym(n, maxrow)
    lit = O.nr_linbcg_sym(sa, ija, S.bvec(n), K, 0)
    rev = O.nr_linbcg_sym(sa, ija, S.bvec(n), K, 1)
    return float(np.max(np.abs(rev - lit)) / np.max(np.abs(lit)))


# --------------------------------------------------------------- the device
@pytest.fixture
def L():
    lib = P.lib()
    lib.perc_nr_bind(None, None, 0)
    lib.perc_nr_set_dot_order(DOT_LITERAL)
    try:
        yield lib
    finally:
        lib.perc_nr_bind(None, None, 0)
        lib.perc_nr_set_dot_order(DOT_LITERAL)


def dev_spmv(L, entry, sa, ija, x):
    """y of dsprsax_ / dsprstx_ (bare arrays) or atimes0 / atimes1 (the same
    arrays bound)"""
    n = int(ija[0]) - 2
    x = np.array(x, dtype=np.float64, copy=True)
    y = np.full(n, np.nan)
    nn = C.c_int(n)
    if entry in ("dsprsax_", "dsprstx_"):
        getattr(L, entry)(sa.ctypes.data, ija.ctypes.data, x.ctypes.data, y.ctypes.data,
                          C.byref(nn))
    else:
        tr = C.c_int(int(entry[-1]))
        L.perc_nr_bind(sa.ctypes.data, ija.ctypes.data, len(sa))
        try:
            L.atimes_(C.byref(nn), x.ctypes.data, y.ctypes.data, C.byref(tr))
        finally:
            L.perc_nr_bind(None, None, 0)
    assert L.perc_nr_status() == 0, (entry, L.perc_nr_status())
    return y


def dev_solve(L, sa, ija, b, x0, itol, tol=TOL, itmax=ITMAX):
    """linbcg_ on the bound (sa, ija): (x, iter, err, status)"""
    n = int(ija[0]) - 2
    b = np.array(b, dtype=np.float64, copy=True)
    x = np.array(x0, dtype=np.float64, copy=True)
    nn, it_, mx, it = C.c_int(n), C.c_int(itol), C.c_int(itmax), C.c_int(-1)
    tl, err = C.c_double(tol), C.c_double(-1.0)
    L.perc_nr_bind(sa.ctypes.data, ija.ctypes.data, len(sa))
    try:
        L.linbcg_(C.byref(nn), b.ctypes.data, x.ctypes.data, C.byref(it_), C.byref(tl),
                  C.byref(mx), C.byref(it), C.byref(err))
    finally:
        L.perc_nr_bind(None, None, 0)
    return x, it.value, err.value, L.perc_nr_status()


def assert_solve_is(got, want, what):
    x, it, err, st = got
    wx, wit, werr = want
    assert st == 0, (what, st)
    assert it == wit, (what, it, wit)
    assert bits(err)[0] == bits(werr)[0], (what, err, werr)
    bad = np.nonzero(bits(x) != bits(wx))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], x[bad[:5]], wx[bad[:5]])


# ------------------------------------------------------------------ products
def check_products(L, sa, ija, x, what):
    ax, atx = O.nr_ax(sa, ija, x), O.nr_ax(sa, ija, x, transpose=True)
    out = {}
    for entry, want in (("dsprsax_", ax), ("dsprstx_", atx), ("atimes0", ax), ("atimes1", atx)):
        y = dev_spmv(L, entry, sa, ija, x)
        bad = np.nonzero(bits(y) != bits(want))[0]
        assert len(bad) == 0, (what, entry, len(bad), bad[:5], y[bad[:5]], want[bad[:5]])
        out[entry] = y
    return out, ax, atx


@pytest.mark.parametrize("maxrow", [4, 6, 11])
@pytest.mark.parametrize("n", SPMV_N)
def test_products_symmetric(L, n, maxrow):
    """rows of <= 4, <= 6 and up to 11 entries (k_spmv<4>, <6>, <0>), empty
    rows, sizes around 64 / 256 / 512 and past 64 workgroups"""
    sa, ija = sym(n, maxrow)
    check_products(L, sa, ija, S.xvec(n), (n, maxrow))


@pytest.mark.parametrize("n,maxrow", S.GENERAL)
def test_products_general_take_the_explicit_transpose(L, n, maxrow):
    sa, ija = gen(n, maxrow)
    out, ax, atx = check_products(L, sa, ija, S.xvec(n), (n, maxrow))
    # the transposed product is not the plain one
    assert not np.array_equal(bits(out["dsprstx_"]), bits(out["dsprsax_"]))
    assert not np.array_equal(bits(out["atimes1"]), bits(out["atimes0"]))


@pytest.mark.parametrize("n,seed", S.ALMOST_SYM)
def test_products_of_a_matrix_one_ulp_from_symmetric(L, n, seed):
    """symmetric pattern, one value an ulp off: dsprstx_ must form A' x, not
    take the symmetric shortcut to A x"""
    rows, diag, (i, j) = S.almost_sym(n, seed)
    sa, ija = S.to_nr(rows, diag)
    x = S.xvec(n)
    out, ax, atx = check_products(L, sa, ija, x, (n, seed))
    diff = np.nonzero(bits(out["dsprstx_"]) != bits(ax))[0]
    assert len(diff) > 0 and set(diff) <= {i, j}, diff


# ------------------------------------------------------ linbcg_, literal order
@pytest.mark.parametrize("which", STARTS)
@pytest.mark.parametrize("n,maxrow,itol", LITERAL_CASES)
def test_linbcg_literal_is_the_oracle_bitwise(L, n, maxrow, itol, which):
    sa, ija = sym(n, maxrow)
    want = ref_solve(n, maxrow, itol, which)
    assert want[1] <= 120 and want[2] <= TOL  # (the oracle converged)
    got = dev_solve(L, sa, ija, S.bvec(n), start(n, which), itol)
    assert_solve_is(got, want, (n, maxrow, itol, which))


@pytest.mark.parametrize("which", STARTS)
@pytest.mark.parametrize("itmax", [0, 1, 2, 7])
def test_linbcg_runs_itmax_plus_one_iterations(L, itmax, which):
    """the loop is `while (iter <= itmax)` (bondc.f:780): itmax + 1
    iterations when the tolerance never stops it; the early iterates bitwise"""
    n, maxrow = 1500, 11
    sa, ija = sym(n, maxrow)
    want = ref_solve(n, maxrow, 2, which, tol=1e-300, itmax=itmax)
    assert want[1] == itmax + 1
    got = dev_solve(L, sa, ija, S.bvec(n), start(n, which), 2, tol=1e-300, itmax=itmax)
    assert got[1] == itmax + 1
    assert_solve_is(got, want, (itmax, which))


@pytest.mark.parametrize("n,maxrow,itol", [(257, 6, 2), (1500, 11, 2), (1500, 11, 1), (257, 6, 3)])
def test_linbcg_from_minus_zero(L, n, maxrow, itol):
    """x = -0.0 everywhere is not linbcg_'s 'x is zero' (it keeps the
    caller's x and forms r = b - A x): the oracle's result for that start"""
    sa, ija = sym(n, maxrow)
    x0 = np.full(n, -0.0)
    assert np.all(np.signbit(x0))
    want = O.nr_linbcg(sa, ija, S.bvec(n), x0, itol, TOL, ITMAX)
    got = dev_solve(L, sa, ija, S.bvec(n), x0, itol)
    assert_solve_is(got, want, (n, maxrow, itol))


def nan_canonical(a):
    """bit view with every NaN the same word.  IEEE 754 leaves the sign and
    payload of a NaN that an operation creates unspecified, and the two
    machines differ: the 0/0 of err = |r| / bnrm is 0xfff8... on x86 and
    0x7ff8... on the GPU (the NaNs of x, carried through the updates, agree).
    Every other value, infinities and signed zeros included, keeps its bits."""
    a = np.array(a, dtype=np.float64, copy=True)
    a[np.isnan(a)] = np.nan
    return bits(a)


@pytest.mark.parametrize("itol", [1, 2])
def test_linbcg_zero_rhs_nonzero_start(L, itol):
    """b = 0 from x0 != 0: bnrm = 0, err = |r| / 0 until r underflows; what
    the oracle returns -- iterations, err, every x(j), NaN / inf pattern
    included -- through bit views"""
    n, maxrow = 257, 6
    sa, ija = sym(n, maxrow)
    x0 = start(n, "normal")
    wx, wit, werr = O.nr_linbcg(sa, ija, np.zeros(n), x0, itol, TOL, ITMAX)
    x, it, err, st = dev_solve(L, sa, ija, np.zeros(n), x0, itol)
    print("zero rhs itol %d: oracle iter %d err %r nan %d inf %d x(1) %#x; device iter %d err %r "
          "nan %d inf %d x(1) %#x" % (itol, wit, werr, np.isnan(wx).sum(), np.isinf(wx).sum(),
                                      int(bits(wx)[0]), it, err, np.isnan(x).sum(),
                                      np.isinf(x).sum(), int(bits(x)[0])))
    assert st == 0
    assert it == wit
    assert nan_canonical(err)[0] == nan_canonical(werr)[0], (err, werr)
    assert np.array_equal(np.isnan(x), np.isnan(wx)) and np.array_equal(np.isinf(x), np.isinf(wx))
    assert np.array_equal(nan_canonical(x), nan_canonical(wx))


# --------------------------------------------------------- linbcg_, fast order
@pytest.mark.parametrize("which", STARTS)
@pytest.mark.parametrize("n,maxrow,itol", FAST_CASES)
def test_linbcg_fast_order_at_a_fixed_iteration(L, n, maxrow, itol, which):
    """K = half the oracle's converged count, no tolerance stop: the fast
    order's x against the literal x, max |dx| / max |x|, within 1.5 x the
    oracle's own re-association spread at the same K (floor 1e-10)"""
    sa, ija = sym(n, maxrow)
    K = max(1, ref_solve(n, maxrow, itol, which)[1] // 2)
    xlit, itlit, _ = ref_solve(n, maxrow, itol, which, tol=1e-300, itmax=K - 1)
    assert itlit == K
    spread = ref_spread(n, maxrow, K)
    bar = max(1e-10, 1.5 * spread)
    assert L.perc_nr_set_dot_order(DOT_FAST) == 0
    x, it, err, st = dev_solve(L, sa, ija, S.bvec(n), start(n, which), itol, tol=1e-300,
                               itmax=K - 1)
    assert st == 0 and it == K, (st, it, K)
    dev = float(np.max(np.abs(x - xlit)) / np.max(np.abs(xlit)))
    msg = "n=%d maxrow=%d itol=%d start=%s K=%d: oracle spread %.3g, device %.3g, bar %.3g" % (
        n, maxrow, itol, which, K, spread, dev, bar)
    print("FAST " + msg)
    assert dev <= bar, msg


@pytest.mark.parametrize("which", STARTS)
@pytest.mark.parametrize("n,maxrow,itol", FAST_CASES)
def test_linbcg_fast_order_converges(L, n, maxrow, itol, which):
    sa, ija = sym(n, maxrow)
    wx, wit, werr = ref_solve(n, maxrow, itol, which)
    assert L.perc_nr_set_dot_order(DOT_FAST) == 0
    x, it, err, st = dev_solve(L, sa, ija, S.bvec(n), start(n, which), itol)
    assert st == 0
    assert err <= TOL, err
    assert abs(it - wit) <= 1, (it, wit)


# ------------------------------------------------------------- context reuse
def test_one_context_over_changing_matrices(L):
    """The device context of the NR layer is reallocated only when N changes
    or the entry count grows: one sequence of matrices -- same N with fewer
    entries, same N with more, smaller, larger, tiny -- with products of a
    general matrix of the same N and solves in between; every result bitwise
    what the call gives on its own (the tests above: the oracle's)."""
    seq = [(1500, 11, None), (1500, 4, None), (1500, 11, 4242), (257, 6, None), (20001, 11, None),
           (3, 2, None)]
    more = S.nnz_of(sym(1500, 11, 4242)[1]) > S.nnz_of(sym(1500, 4)[1]) > 0
    assert more and S.nnz_of(sym(1500, 4)[1]) < S.nnz_of(sym(1500, 11)[1])
    for step, (n, maxrow, seed) in enumerate(seq):
        sa, ija = sym(n, maxrow, seed)
        gsa, gija = gen(n, 9)
        x = S.xvec(n)
        what = (step, n, maxrow)

        def same(y, want, tag):
            assert np.array_equal(bits(y), bits(want)), (what, tag)

        same(dev_spmv(L, "dsprsax_", sa, ija, x), O.nr_ax(sa, ija, x), "dsprsax_")
        same(dev_spmv(L, "dsprstx_", gsa, gija, x), O.nr_ax(gsa, gija, x, True), "dsprstx_ general")
        assert_solve_is(dev_solve(L, sa, ija, S.bvec(n), start(n, "normal"), 2),
                        ref_solve(n, maxrow, 2, "normal", seed=seed), (what, "itol 2"))
        same(dev_spmv(L, "dsprsax_", gsa, gija, x), O.nr_ax(gsa, gija, x), "dsprsax_ general")
        assert_solve_is(dev_solve(L, sa, ija, S.bvec(n), start(n, "zero"), 3),
                        ref_solve(n, maxrow, 3, "zero", seed=seed), (what, "itol 3"))
        same(dev_spmv(L, "atimes1", sa, ija, x), O.nr_ax(sa, ija, x, True), "atimes_(1)")
        assert_solve_is(dev_solve(L, sa, ija, S.bvec(n), start(n, "zero"), 2),
                        ref_solve(n, maxrow, 2, "zero", seed=seed), (what, "itol 2 from 0"))
