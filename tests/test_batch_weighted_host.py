"""perc_batch_weighted_supported (host-only): which lattices the weighted
batch kernel (k_batch_cond_w: p and the rows' slot values in LDS, 4 rows per
thread) takes per kind -- every lattice of the reference's ensembles, up to
where its LDS plan ends -- and the entry points' declarations."""
import itertools
import os
import re

import pytest

from percolation_amd import _lib as L
from percolation_amd import api

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (L.BOND, L.SITE, L.SITEBOND)
SIZES = (3, 4, 10, 31, 50, 64, 90, 91, 130, 200, 1000, 2730)
NEW = ("perc_batch_weighted_supported", "perc_batch_cond_weighted", "perc_batch_twister")
# at m = 50 the arena is 40 N + 25 488 bytes (square, 4 slots) or
# 56 N + 25 488 (triangular, 6 slots) with the static 2 048 included, N = 50
# (n - 2), against 163 840: the last lattices that fit are 50 x 71 (163 488)
# and 50 x 51 (162 688)
FIRST_REFUSED = {L.SQUARE: 72, L.TRIANGULAR: 52}


@pytest.mark.parametrize("kind", KINDS)
def test_accepts_the_reference_ensembles(kind):
    lib = L.lib()
    for lattice, size, pbc in itertools.product((L.SQUARE, L.TRIANGULAR), (10, 20, 30, 40, 50), (0, 1)):
        assert api.batch_weighted_supported(kind, lattice, size, size, pbc) is True, (kind, lattice, size, pbc)
        assert lib.perc_batch_weighted_supported(kind, lattice, size, size, pbc) == 1
    assert api.batch_weighted_supported(kind, L.TRIANGULAR, 12, 10, 1)
    assert api.batch_weighted_supported(kind, L.SQUARE, 3, 3, 0)


@pytest.mark.parametrize("kind", KINDS)
def test_refusals(kind):
    for lat in [(0, 10, 2, 0), (1, 10, 2, 1),    # n = 2
                (0, 2, 10, 0),                   # m = 2
                (1, 11, 10, 0), (1, 49, 50, 1),  # odd m on the triangular lattice
                (0, 128, 128, 0), (1, 128, 128, 1), (0, 64, 130, 0)]:
        assert api.batch_weighted_supported(kind, *lat) is False, (kind, lat)
    assert not api.batch_weighted_supported(L.BONDSITE, 0, 10, 10, 0)
    assert not api.batch_weighted_supported(-1, 0, 10, 10, 0)
    assert not api.batch_weighted_supported(kind, 2, 10, 10, 0)
    assert not api.batch_weighted_supported(kind, 0, 0, 10, 0)
    assert not api.batch_weighted_supported(kind, 0, 1 << 20, 1 << 20, 0)


@pytest.mark.parametrize("pbc", (0, 1))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lattice", (L.SQUARE, L.TRIANGULAR))
def test_first_refused_is_what_the_lds_plan_predicts(lattice, kind, pbc):
    first = next(n for n in range(3, 200) if not api.batch_weighted_supported(kind, lattice, 50, n, pbc))
    assert first == FIRST_REFUSED[lattice]
    # and nothing larger comes back
    assert not any(api.batch_weighted_supported(kind, lattice, 50, n, pbc) for n in range(first, 200))


@pytest.mark.parametrize("kind", KINDS)
def test_never_accepts_what_the_large_kernel_refuses(kind):
    seen = {True: 0, False: 0}
    for lattice, m, n, pbc in itertools.product((L.SQUARE, L.TRIANGULAR), SIZES, SIZES, (0, 1)):
        w = api.batch_weighted_supported(kind, lattice, m, n, pbc)
        if w:
            assert api.batch_large_supported(kind, lattice, m, n, pbc), (kind, lattice, m, n, pbc)
            assert (n - 2) * m <= 4096 and m >= 3 and n >= 3
        seen[w] += 1
    assert seen[True] > 20 and seen[False] > 20


def test_symbols_declared():
    """the entry points are in the library, in SIGNATURES, in the header and
    in the Fortran interfaces"""
    lib = L.lib()
    header = open(os.path.join(REPO, "include", "perc.h")).read()
    f90 = open(os.path.join(REPO, "percolation_amd", "fortran", "perc_mod.f90")).read()
    for name in NEW:
        assert name in L.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"\bint %s\(" % name, header), name
        assert "bind(C, name='%s')" % name in f90, name
    assert L.SIGNATURES["perc_batch_weighted_supported"][1] == L.SIGNATURES["perc_batch_cond_supported"][1]
    # perc_batch_cond's arguments with the four weight arguments before `solve`
    a, b = L.SIGNATURES["perc_batch_cond_weighted"][1], L.SIGNATURES["perc_batch_cond"][1]
    assert a[:11] == b[:11] and a[15:] == b[11:] and len(a) == len(b) + 4
    import percolation_amd as P
    assert P.batch_weighted_supported is api.batch_weighted_supported
    assert hasattr(api.Context, "batch_twister")


def test_cond_curve_argument_checks():
    with pytest.raises(ValueError):
        api.cond_curve(0, 10, 10, 0, condtype=3, numtrials=0)
    with pytest.raises(ValueError):
        api.cond_curve(0, 10, 10, 0, condtype=2, large=True, numtrials=0)
