"""Matrices in Numerical Recipes row-indexed storage for the NR drop-in's
tests (test_nr_general_host.py, test_nr_general.py) -- TEST INFRASTRUCTURE
ONLY, NumPy only, every generator deterministic in its seed.

A matrix is (rows, diag): rows[i] = (cols, vals), the off-diagonals of row i
as 0-based ascending int columns and float64 values; diag the n diagonal
entries.  to_nr() gives the (sa, ija) a Fortran caller holds (bondc.f:723-746:
sa(1..n) the diagonal, ija(1) = n+2, ija(i+1) = one past row i's last entry,
columns 1-based ascending); dense() the same matrix as an n x n array.
"""
import numpy as np

NEAR = 40  # |i - j| of a "near" partner


def _partner(rng, n, i, near):
    if near:
        lo, hi = max(0, i - NEAR), min(n - 1, i + NEAR)
        return int(rng.integers(lo, hi + 1))
    return int(rng.integers(0, n))


def sym_spd(n, maxrow, seed, leak=0.05, empty=()):
    """Bitwise-symmetric, strictly diagonally dominant (so SPD), rows of 0 ..
    maxrow off-diagonals: every row draws a target count, then partners --
    alternately near (|i - j| <= 40) and anywhere -- until it has that many
    (a partner's row may so pass its own target, never maxrow).  Values are
    uniform in -[0.1, 2], the same double at (i, j) and (j, i); the diagonal
    is sum |off| + leak * U[0.5, 1.5].  Rows in `empty` keep only their
    diagonal."""
    rng = np.random.default_rng(seed)
    maxrow = min(maxrow, n - 1)
    empty = set(int(e) % n for e in empty) if n > 0 else set()
    target = rng.integers(0, maxrow + 1, size=n)
    adj = [dict() for _ in range(n)]
    for i in range(n):
        if i in empty:
            continue
        tries = 0
        while len(adj[i]) < target[i] and tries < 20 * (maxrow + 1):
            tries += 1
            j = _partner(rng, n, i, near=(tries % 2 == 1))
            if j == i or j in empty or j in adj[i] or len(adj[j]) >= maxrow:
                continue
            v = -float(rng.uniform(0.1, 2.0))
            adj[i][j] = v
            adj[j][i] = v
    rows, diag = [], np.zeros(n)
    for i in range(n):
        cols = np.array(sorted(adj[i]), dtype=np.int64)
        vals = np.array([adj[i][c] for c in cols], dtype=np.float64)
        rows.append((cols, vals))
        diag[i] = float(np.sum(np.abs(vals))) + leak * float(rng.uniform(0.5, 1.5))
    return rows, diag


def general(n, maxrow, seed):
    """Non-symmetric pattern and values: every row 0 .. maxrow distinct
    random columns, values +-[0.1, 2]; about one row in eight (and, for n >
    10, the first and the last) empty; the diagonal +-[0.5, 3]."""
    rng = np.random.default_rng(seed)
    maxrow = min(maxrow, n - 1)
    rows = []
    for i in range(n):
        cnt = int(rng.integers(0, maxrow + 1))
        if rng.random() < 0.125 or (n > 10 and i in (0, n - 1)):
            cnt = 0
        others = np.delete(np.arange(n), i)
        cols = np.sort(rng.choice(others, size=cnt, replace=False)).astype(np.int64)
        vals = rng.uniform(0.1, 2.0, size=cnt) * rng.choice([-1.0, 1.0], size=cnt)
        rows.append((cols, vals.astype(np.float64)))
    diag = rng.uniform(0.5, 3.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    return rows, diag


def almost_sym(n, seed):
    """sym_spd(n, 6, seed) with exactly one off-diagonal value moved by one
    ulp: the pattern stays symmetric, the values do not.  Returns (rows,
    diag, (i, j)): the entry moved is A(i, j); A(j, i) keeps its value."""
    rows, diag = sym_spd(n, 6, seed, empty=(0, n - 1) if n > 10 else ())
    rng = np.random.default_rng(seed + 1)
    cand = [i for i in range(n) if len(rows[i][0]) > 0]
    i = cand[int(rng.integers(0, len(cand)))]
    k = int(rng.integers(0, len(rows[i][0])))
    vals = rows[i][1].copy()
    vals[k] = np.nextafter(vals[k], 0.0)
    rows[i] = (rows[i][0], vals)
    return rows, diag, (i, int(rows[i][0][k]))


def nnz(rows):
    return int(sum(len(c) for c, _ in rows))


def nnz_of(ija):
    """the off-diagonal count an ija array declares"""
    n = int(ija[0]) - 2
    return int(ija[n]) - (n + 2)


def to_nr(rows, diag, pad=0):
    """(sa, ija): float64 / int32 arrays of n + 1 + nnz (+ pad) entries."""
    n = len(diag)
    k = n + 1 + nnz(rows)
    sa, ija = np.zeros(k + pad), np.zeros(k + pad, dtype=np.int32)
    sa[:n] = diag
    ija[0] = n + 2
    at = n + 1
    for i, (cols, vals) in enumerate(rows):
        assert np.all(np.diff(cols) > 0)
        sa[at:at + len(cols)] = vals
        ija[at:at + len(cols)] = cols + 1
        at += len(cols)
        ija[i + 1] = at + 1
    return sa, ija


def dense(rows, diag):
    n = len(diag)
    a = np.zeros((n, n))
    a[np.arange(n), np.arange(n)] = diag
    for i, (cols, vals) in enumerate(rows):
        a[i, cols] = vals
    return a


def edge_rows(n):
    """the rows the suites' sym_spd cases keep empty: the first and the last
    (a row without entries at the very end of the storage), for n > 10"""
    return (0, n - 1) if n > 10 else ()


# ------------------------------------------------- the cases both suites use
def seed_of(n, maxrow):
    return 1200 + n + maxrow


def xvec(n, salt=0):
    """the standard-normal vector of size n (products' x, solves' start)"""
    return np.random.default_rng(9000 + n + salt).standard_normal(n)


def bvec(n):
    """the standard-normal right-hand side of size n"""
    return np.random.default_rng(5000 + n).standard_normal(n)


# general(n, maxrow, seed_of(n, maxrow)): the explicit-transpose cases
GENERAL = [(n, maxrow) for maxrow in (3, 6, 9) for n in (2, 257, 1500)]
# almost_sym(n, seed): seeds at which the one ulp shows in the oracle's
# products with xvec(n) (it can round away: test_almost_sym_moves_one_value_by_one_ulp)
ALMOST_SYM = [(65, 70), (257, 70), (1500, 70)]
