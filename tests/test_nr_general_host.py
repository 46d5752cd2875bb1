"""The NR drop-in (perc_nr.cpp: sprsin_, dsprsax_, dsprstx_, atimes_, asolve_,
snrm_, linbcg_) on general matrices: everything that is decided on the host.

No test here needs a GPU.  The routines that run on the host (sprsin_,
snrm_, asolve_) are compared bitwise with plain restatements of
Square/bondc.f:723-746, 855-884; the statuses that the layer decides before
any device call (PERC_EMISMATCH, PERC_EINVAL, PERC_EITOL, PERC_ESTATE,
PERC_ENMAX) are asserted exactly -- without a device they differ from the
PERC_ENODEV a well-formed call ends with.  The oracle's dsprsax / dsprstx,
the reference of test_nr_general.py, are checked against a dense product in
extended precision first, so that suite's reference is independent of the
sparse storage it reads.
"""
import ctypes as C

import numpy as np
import pytest

import nr_systems as S
import oracle_lib as O
import percolation_amd as P

EINVAL, ENMAX, EITOL, EMISMATCH, ENODEV, ESTATE = -1, -4, -5, -6, -8, -9
DOT_FAST, DOT_LITERAL = 0, 1
# a well-formed call passes the host checks: it ends with 0 on a device and
# with PERC_ENODEV without one
PASSED = (0, ENODEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture
def L():
    lib = P.lib()
    lib.perc_nr_bind(None, None, 0)
    try:
        yield lib
    finally:
        lib.perc_nr_bind(None, None, 0)
        lib.perc_nr_set_dot_order(DOT_LITERAL)


def call_spmv(L, name, sa, ija, x, n):
    y = np.zeros(n)
    nn = C.c_int(n)
    getattr(L, name)(sa.ctypes.data, ija.ctypes.data, x.ctypes.data, y.ctypes.data, C.byref(nn))
    return L.perc_nr_status()


def call_atimes(L, x, n, itrnsp):
    y = np.zeros(n)
    nn, tr = C.c_int(n), C.c_int(itrnsp)
    L.atimes_(C.byref(nn), x.ctypes.data, y.ctypes.data, C.byref(tr))
    return L.perc_nr_status()


def call_linbcg(L, n, itol=2, b=None, x=None):
    b = np.ones(n) if b is None else b
    x = np.zeros(n) if x is None else x
    nn, it_, itmax, it = C.c_int(n), C.c_int(itol), C.c_int(100), C.c_int(-7)
    tol, err = C.c_double(1e-10), C.c_double()
    L.linbcg_(C.byref(nn), b.ctypes.data, x.ctypes.data, C.byref(it_), C.byref(tol),
              C.byref(itmax), C.byref(it), C.byref(err))
    return L.perc_nr_status()


# --------------------------------------------------------------- generators
@pytest.mark.parametrize("n,maxrow", [(1, 0), (2, 1), (3, 2), (65, 4), (257, 6), (513, 11),
                                      (1500, 4), (1500, 6), (1500, 11)])
def test_sym_spd_is_what_it_says(n, maxrow):
    rows, diag = S.sym_spd(n, maxrow, S.seed_of(n, maxrow), empty=S.edge_rows(n))
    a = S.dense(rows, diag)
    assert np.array_equal(bits(a), bits(a.T))
    cnt = np.array([len(c) for c, _ in rows])
    assert cnt.max() == min(maxrow, n - 1)
    off = a - np.diag(diag)
    assert np.all(off <= 0) and np.all((off == 0) | ((off <= -0.1) & (off >= -2.0)))
    assert np.all(diag > np.abs(off).sum(axis=1))
    if n > 10:
        assert cnt[0] == 0 and cnt[-1] == 0
    sa, ija = S.to_nr(rows, diag)
    assert ija[0] == n + 2 and ija[n] - 1 == len(sa) == n + 1 + S.nnz(rows)
    # the oracle's view of the storage is the dense matrix
    x = np.random.default_rng(n).standard_normal(n)
    assert np.allclose(O.nr_ax(sa, ija, x), a @ x, rtol=0, atol=1e-12 * np.abs(a).sum(axis=1).max())


def test_almost_sym_moves_one_value_by_one_ulp():
    for n, seed in S.ALMOST_SYM:
        rows, diag, (i, j) = S.almost_sym(n, seed)
        a = S.dense(rows, diag)
        assert np.array_equal(a != 0, (a != 0).T)
        d = np.argwhere(bits(a) != bits(a.T))
        assert sorted(map(tuple, d)) == sorted([(i, j), (j, i)])
        assert abs(int(bits(a[i, j])[0]) - int(bits(a[j, i])[0])) == 1
        # the one ulp shows in the oracle's products, in rows i or j only
        sa, ija = S.to_nr(rows, diag)
        x = S.xvec(n)
        diff = np.nonzero(bits(O.nr_ax(sa, ija, x)) != bits(O.nr_ax(sa, ija, x, True)))[0]
        assert len(diff) > 0 and set(diff) <= {i, j}


# ------------------------------------------------------ oracle independence
@pytest.mark.parametrize("n,maxrow", S.GENERAL)
def test_oracle_products_against_the_dense_matrix(n, maxrow):
    """or_dsprsax / or_dsprstx against A x and A' x formed from the dense
    matrix in np.longdouble.  A sum of k = rowlen + 1 products in double
    carries at most k roundings of at most half an ulp of a partial sum
    each, every partial sum <= sum |a||x|: the bound is k ulps of that."""
    rows, diag = S.general(n, maxrow, S.seed_of(n, maxrow))
    sa, ija = S.to_nr(rows, diag)
    a = S.dense(rows, diag)
    x = S.xvec(n)
    al, xl = a.astype(np.longdouble), x.astype(np.longdouble)
    for tr in (False, True):
        m = al.T if tr else al
        want = m @ xl
        mag = (np.abs(m) @ np.abs(xl)).astype(np.float64)
        k = (m != 0).sum(axis=1)  # off-diagonals + the diagonal
        got = O.nr_ax(sa, ija, x, transpose=tr)
        err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
        assert np.all(err <= k * np.spacing(mag)), (tr, float(np.max(err / np.spacing(mag))))
    ax, atx = O.nr_ax(sa, ija, x), O.nr_ax(sa, ija, x, True)
    if n > 2 or S.nnz(rows) > 0:
        # the transpose is another product altogether, not a rounding apart
        assert np.max(np.abs(ax - atx)) > 0.1 * np.max(np.abs(ax))


# ------------------------------------------------------------------ sprsin_
def sprsin_restated(a, n, thresh, nmax, sa, ija):
    """Square/bondc.f:723-746 on a(np, np) (a[i, j] = a(i+1, j+1)); where the
    reference `pause`s ('nmax too small in sprsin') it stops: returns False
    with sa / ija as written until then."""
    for j in range(1, n + 1):
        sa[j - 1] = a[j - 1, j - 1]
    ija[0] = n + 2
    k = n + 1
    for i in range(1, n + 1):
        for j in range(1, n + 1):
            if abs(a[i - 1, j - 1]) >= thresh:
                if i != j:
                    k = k + 1
                    if k > nmax:
                        return False
                    sa[k - 1] = a[i - 1, j - 1]
                    ija[k - 1] = j
        ija[i] = k + 1
    return True


def run_sprsin(L, a, n, thresh, nmax, size):
    """sprsin_ on the column-major a; sa / ija of `size` >= nmax entries,
    pre-filled so that every entry the routine leaves alone shows."""
    npd = a.shape[0]
    af = np.asfortranarray(a, dtype=np.float64)
    sa, ija = np.full(size, -777.25), np.full(size, -777, dtype=np.int32)
    nn, np_, nm, th = C.c_int(n), C.c_int(npd), C.c_int(nmax), C.c_double(thresh)
    L.sprsin_(af.ctypes.data, C.byref(nn), C.byref(np_), C.byref(th), C.byref(nm),
              sa.ctypes.data, ija.ctypes.data)
    wsa, wija = np.full(size, -777.25), np.full(size, -777, dtype=np.int32)
    ok = sprsin_restated(a, n, thresh, nmax, wsa, wija)
    return L.perc_nr_status(), sa, ija, ok, wsa, wija


def sprsin_matrix(n, npd, seed, thresh):
    """general(n) in a padded np x np array (the padding non-zero: never
    read), with some off-diagonals of magnitude exactly thresh (kept: the
    test is >=) and some just below it (dropped)."""
    rows, diag = S.general(n, 5, seed)
    a = np.full((npd, npd), 9.5)
    a[:n, :n] = S.dense(rows, diag)
    rng = np.random.default_rng(seed)
    for _ in range(2 * n):
        i, j = rng.integers(0, n, size=2)
        if i != j:
            a[i, j] = rng.choice([thresh, -thresh, np.nextafter(thresh, 0.0), -np.nextafter(thresh, 0.0)])
    return a


@pytest.mark.parametrize("n,npd", [(1, 1), (1, 3), (2, 2), (7, 7), (7, 10), (40, 64)])
def test_sprsin_is_the_reference_loop(L, n, npd):
    thresh = 0.25
    a = sprsin_matrix(n, npd, 100 + n, thresh)
    need = n + 1 + int(np.sum((np.abs(a[:n, :n]) >= thresh) & ~np.eye(n, dtype=bool)))
    if n >= 7:
        off = a[:n, :n][~np.eye(n, dtype=bool)]
        assert np.any(np.abs(off) == thresh) and np.any(np.abs(off) == np.nextafter(thresh, 0.0))
    # nmax the exact need: status 0, the reference's storage bitwise
    st, sa, ija, ok, wsa, wija = run_sprsin(L, a, n, thresh, need, need + 8)
    assert st == 0 and ok
    assert np.array_equal(ija, wija) and np.array_equal(bits(sa), bits(wsa))
    assert ija[n] - 1 == need
    if need > n + 1:
        # one less: PERC_ENMAX; what was written before the overflow stands
        st, sa, ija, ok, wsa, wija = run_sprsin(L, a, n, thresh, need - 1, need + 8)
        assert st == ENMAX and not ok
        assert np.array_equal(ija, wija) and np.array_equal(bits(sa), bits(wsa))
        # and the status is not sticky
        assert run_sprsin(L, a, n, thresh, need, need + 8)[0] == 0


def test_sprsin_with_every_offdiagonal_below_thresh(L):
    n = 9
    a = np.random.default_rng(4).uniform(-0.2, 0.2, size=(n, n))
    a[np.arange(n), np.arange(n)] = 0.0  # (a zero diagonal is still stored)
    st, sa, ija, ok, wsa, wija = run_sprsin(L, a, n, 0.25, n + 1, n + 9)
    assert st == 0 and ok
    assert np.array_equal(ija, wija) and np.array_equal(bits(sa), bits(wsa))
    assert np.all(ija[:n + 1] == n + 2)


# ---------------------------------------------------------- snrm_ / asolve_
def serial_snrm(x, itol):
    if itol <= 3:
        s = 0.0
        for v in x:
            s = s + v * v
        return np.sqrt(s)
    return float(np.max(np.abs(x)))


@pytest.mark.parametrize("n", [1, 2, 64, 1001])
@pytest.mark.parametrize("itol", [1, 2, 3, 4])
def test_snrm_is_the_serial_sum_or_max(L, n, itol):
    x = np.random.default_rng(n + itol).standard_normal(n) * 10.0 ** np.random.default_rng(n).integers(-8, 8, n)
    nn, it_ = C.c_int(n), C.c_int(itol)
    got = L.snrm_(C.byref(nn), x.ctypes.data, C.byref(it_))
    assert bits(got)[0] == bits(serial_snrm(x, itol))[0]


@pytest.mark.parametrize("itrnsp", [0, 1])
def test_asolve_divides_by_the_bound_diagonal(L, itrnsp):
    n = 257
    rows, diag = S.general(n, 6, 9)  # (a diagonal of either sign)
    sa, ija = S.to_nr(rows, diag)
    b = S.xvec(n)
    x = np.zeros(n)
    nn, tr = C.c_int(n), C.c_int(itrnsp)
    L.asolve_(C.byref(nn), b.ctypes.data, x.ctypes.data, C.byref(tr))
    assert L.perc_nr_status() == ESTATE and np.all(x == 0)
    L.perc_nr_bind(sa.ctypes.data, ija.ctypes.data, len(sa))
    L.asolve_(C.byref(nn), b.ctypes.data, x.ctypes.data, C.byref(tr))
    assert np.array_equal(bits(x), bits(b / sa[:n]))


# ------------------------------------------------- statuses set on the host
def good_system(n=65, maxrow=4, pad=0):
    rows, diag = S.sym_spd(n, maxrow, S.seed_of(n, maxrow), empty=S.edge_rows(n))
    sa, ija = S.to_nr(rows, diag, pad=pad)
    return sa, ija, n + 1 + S.nnz(rows)


def test_first_index_must_be_n_plus_2(L):
    sa, ija, k = good_system()
    n, x = 65, S.xvec(65)
    for bad in (n + 1, n + 3, 0):
        ij = ija.copy()
        ij[0] = bad
        assert call_spmv(L, "dsprsax_", sa, ij, x, n) == EMISMATCH
        assert call_spmv(L, "dsprstx_", sa, ij, x, n) == EMISMATCH
        L.perc_nr_bind(sa.ctypes.data, ij.ctypes.data, k)
        assert call_atimes(L, x, n, 0) == EMISMATCH
        assert call_atimes(L, x, n, 1) == EMISMATCH
        assert call_linbcg(L, n) == EMISMATCH
        L.perc_nr_bind(None, None, 0)
    # a wrong n with good storage is the same mismatch
    assert call_spmv(L, "dsprsax_", sa, ija, x, n - 1) == EMISMATCH
    assert call_spmv(L, "dsprsax_", sa, ija, x, n) in PASSED


@pytest.mark.parametrize("badcol", [0, 66])
def test_column_out_of_range(L, badcol):
    sa, ija, k = good_system()
    n, x = 65, S.xvec(65)
    for at in (n + 1, k - 1, (n + 1 + k) // 2):  # first, last, a middle entry
        ij = ija.copy()
        ij[at] = badcol
        assert call_spmv(L, "dsprsax_", sa, ij, x, n) == EMISMATCH
        assert call_spmv(L, "dsprstx_", sa, ij, x, n) == EMISMATCH
        L.perc_nr_bind(sa.ctypes.data, ij.ctypes.data, k)
        assert call_atimes(L, x, n, 0) == EMISMATCH
        assert call_linbcg(L, n) == EMISMATCH
        L.perc_nr_bind(None, None, 0)


def test_nothing_bound_is_estate(L):
    n, x = 65, S.xvec(65)
    assert call_atimes(L, x, n, 0) == ESTATE
    assert call_atimes(L, x, n, 1) == ESTATE
    assert call_linbcg(L, n) == ESTATE
    y = np.zeros(n)
    nn, tr = C.c_int(n), C.c_int(0)
    L.asolve_(C.byref(nn), x.ctypes.data, y.ctypes.data, C.byref(tr))
    assert L.perc_nr_status() == ESTATE
    assert np.all(y == 0)
    # binding and unbinding leaves nothing bound
    sa, ija, k = good_system()
    L.perc_nr_bind(sa.ctypes.data, ija.ctypes.data, k)
    assert call_atimes(L, x, n, 0) in PASSED
    L.perc_nr_bind(None, None, 0)
    assert call_atimes(L, x, n, 0) == ESTATE


@pytest.mark.parametrize("itol", [0, 5, -1])
def test_illegal_itol_through_the_symbol(L, itol):
    sa, ija, k = good_system()
    L.perc_nr_bind(sa.ctypes.data, ija.ctypes.data, k)
    assert call_linbcg(L, 65, itol=itol) == EITOL
    assert call_linbcg(L, 65, itol=2) in PASSED


def test_linbcg_rejects_a_nonsymmetric_matrix(L):
    for n, maxrow in S.GENERAL:
        rows, diag = S.general(n, maxrow, S.seed_of(n, maxrow))
        if S.nnz(rows) == 0:
            continue  # (a diagonal matrix is symmetric)
        sa, ija = S.to_nr(rows, diag)
        L.perc_nr_bind(sa.ctypes.data, ija.ctypes.data, len(sa))
        assert call_linbcg(L, n) == EINVAL, n
    # a symmetric pattern with one value an ulp off is not symmetric either
    for n, seed in S.ALMOST_SYM:
        rows, diag, _ = S.almost_sym(n, seed)
        sa, ija = S.to_nr(rows, diag)
        L.perc_nr_bind(sa.ctypes.data, ija.ctypes.data, len(sa))
        assert call_linbcg(L, n) == EINVAL, n
        # ... and the matrix it was made from passes
        rows, diag = S.sym_spd(n, 6, seed, empty=S.edge_rows(n))
        sa, ija = S.to_nr(rows, diag)
        L.perc_nr_bind(sa.ctypes.data, ija.ctypes.data, len(sa))
        assert call_linbcg(L, n) in PASSED, n


def test_dot_order_values(L):
    assert L.perc_nr_set_dot_order(7) == EINVAL
    assert L.perc_nr_set_dot_order(-1) == EINVAL
    assert L.perc_nr_set_dot_order(2) == EINVAL  # (the host fold is not an NR order)
    assert L.perc_nr_set_dot_order(DOT_FAST) == 0
    assert L.perc_nr_set_dot_order(DOT_LITERAL) == 0


# ----------------------------------------------- malformed storage, rejected
def test_descending_row_pointers(L):
    """ija(i+1) < ija(i): PERC_EMISMATCH on every entry.  (The columns stay
    in range and ija(n+1) stays put, so nothing else rejects the storage.)"""
    sa, ija, k = good_system()
    n, x = 65, S.xvec(65)
    # a pointer with entries before it (so it can drop and stay >= n+2) and
    # two or more in the row after it
    i = next(i for i in range(1, n) if ija[i - 1] >= n + 4 and ija[i + 1] - ija[i] >= 2)
    for bad in (ija[i - 1] - 1, n + 2):
        ij = ija.copy()
        ij[i] = bad  # below the pointer before it
        assert n + 2 <= ij[i] < ij[i - 1] and ij[n] == ija[n]
        assert call_spmv(L, "dsprsax_", sa, ij, x, n) == EMISMATCH
        assert call_spmv(L, "dsprstx_", sa, ij, x, n) == EMISMATCH
        L.perc_nr_bind(sa.ctypes.data, ij.ctypes.data, k)
        assert call_atimes(L, x, n, 0) == EMISMATCH
        assert call_atimes(L, x, n, 1) == EMISMATCH
        assert call_linbcg(L, n) == EMISMATCH
        L.perc_nr_bind(None, None, 0)
    # the last pointer below the one before it (fewer entries than row n-1 ends with)
    ij = ija.copy()
    ij[n] = ija[n - 1] - 1
    assert call_spmv(L, "dsprsax_", sa, ij, x, n) == EMISMATCH


def test_storage_longer_than_nmax(L):
    """ija(n+1) - 1 > nmax of perc_nr_bind: PERC_EMISMATCH on the bound
    paths.  The arrays are longer than the nmax declared and hold valid
    entries there, so code that did not check would read inside the buffer
    and end with another status."""
    n, pad = 65, 1000
    sa, ija, k = good_system(pad=pad)
    sa[k:] = -0.5
    ija[k:] = 1 + (np.arange(pad) % n)
    x = S.xvec(n)
    L.perc_nr_bind(sa.ctypes.data, ija.ctypes.data, k)
    assert call_atimes(L, x, n, 0) in PASSED
    assert call_linbcg(L, n) in PASSED
    # the declared length one short of what ija(n+1) says
    L.perc_nr_bind(sa.ctypes.data, ija.ctypes.data, k - 1)
    assert call_atimes(L, x, n, 0) == EMISMATCH
    assert call_atimes(L, x, n, 1) == EMISMATCH
    assert call_linbcg(L, n) == EMISMATCH
    # a corrupt last pointer, past the declared length
    for extra in (1, 2, pad):
        ij = ija.copy()
        ij[n] = ija[n] + extra
        L.perc_nr_bind(sa.ctypes.data, ij.ctypes.data, k)
        assert call_atimes(L, x, n, 0) == EMISMATCH, extra
        assert call_atimes(L, x, n, 1) == EMISMATCH, extra
        assert call_linbcg(L, n) == EMISMATCH, extra
    # nmax smaller than the pointer block itself
    L.perc_nr_bind(sa.ctypes.data, ija.ctypes.data, n)
    assert call_atimes(L, x, n, 0) == EMISMATCH
    # the bare-array entries know no nmax: they read what ija says
    ij = ija.copy()
    ij[n] = ija[n] + 2
    assert call_spmv(L, "dsprsax_", sa, ij, x, n) in PASSED


def test_default_nmax_is_the_reference_common(L):
    """perc_nr_bind with nmax <= 0 declares the reference's NMAX = 20000
    (COMMON /mat/, bondc.f:753)."""
    n, size = 100, 20100
    sa, ija = np.full(size, -0.5), np.ones(size, dtype=np.int32)
    sa[:n] = 300.0
    ija[:n + 1] = n + 2
    x = S.xvec(n)
    for last, want in ((20000, PASSED), (20001, (EMISMATCH,))):
        ija[n] = last + 1  # the last row holds every entry up to sa(last): all in column 1
        L.perc_nr_bind(sa.ctypes.data, ija.ctypes.data, 0)
        assert call_atimes(L, x, n, 0) in want, last
