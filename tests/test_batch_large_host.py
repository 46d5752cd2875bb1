"""perc_batch_large_supported (host-only): which lattices the large batch
kernel (k_batch_cond_large: p alone in LDS, 16 rows per thread) takes per
kind -- every lattice perc_batch_cond_supported accepts, and on to 16384
sites (128 x 128, 64 x 256) -- and the default predicates, which it leaves
as they are."""
import itertools
import os
import re

import pytest

from percolation_amd import _lib as L
from percolation_amd import api

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (L.BOND, L.SITE, L.SITEBOND)
# (lattice, m, n, pbc): large predicate, default predicate
TABLE = [
    ((0, 91, 93, 0), True, False),     # N = 8281: a ninth row per thread
    ((0, 128, 128, 0), True, False),   # N = 16128
    ((0, 128, 128, 1), True, False),
    ((0, 64, 256, 0), True, False),    # t = 16384, the cap
    ((0, 256, 64, 0), True, False),
    ((1, 128, 128, 0), True, False),
    ((1, 128, 128, 1), True, False),   # the largest labeling view
    ((0, 129, 128, 0), False, False),  # t = 16512
    ((0, 128, 129, 0), False, False),
    ((0, 10, 2, 0), False, False),     # n < 3
    ((0, 2, 10, 0), False, False),     # m < 3
    ((1, 11, 10, 0), False, False),    # odd m on the triangular lattice
    ((0, 50, 50, 0), True, True),
    ((0, 64, 130, 0), True, True),     # the default kernel's cap, N = 8192
    ((0, 90, 93, 0), True, True),
    ((1, 64, 130, 1), True, True),
    ((0, 3, 3, 0), True, True),
]
SIZES = (3, 4, 10, 31, 50, 64, 90, 91, 130, 200, 1000, 2730)
NEW = ("perc_batch_large_supported", "perc_set_batch_large", "perc_batch_large",
       "perc_ensemble_set_batch_large")


@pytest.mark.parametrize("kind", KINDS)
def test_predicate_table(kind):
    lib = L.lib()
    for lat, large, default in TABLE:
        assert api.batch_large_supported(kind, *lat) is large, (kind, lat)
        assert lib.perc_batch_large_supported(kind, *lat) == (1 if large else 0), (kind, lat)


@pytest.mark.parametrize("kind", KINDS)
def test_default_predicates_unchanged(kind):
    lib = L.lib()
    for lat, _, default in TABLE:
        assert api.batch_cond_supported(kind, *lat) is default, (kind, lat)
        assert lib.perc_batch_cond_supported(kind, *lat) == (1 if default else 0), (kind, lat)
        if kind == L.BOND:
            assert api.batch_supported(*lat) is default, lat
            assert lib.perc_batch_supported(*lat) == (1 if default else 0), lat


@pytest.mark.parametrize("kind", KINDS)
def test_accepts_what_the_default_kernel_accepts(kind):
    """so that the large kernel can be forced wherever the default one runs"""
    seen = {True: 0, False: 0}
    for lattice, m, n, pbc in itertools.product((L.SQUARE, L.TRIANGULAR), SIZES, SIZES, (0, 1)):
        old = api.batch_cond_supported(kind, lattice, m, n, pbc)
        new = api.batch_large_supported(kind, lattice, m, n, pbc)
        if old:
            assert new, (kind, lattice, m, n, pbc)
        if new:
            assert m * n <= 16384 and m >= 3 and n >= 3
        seen[old] += 1
    assert seen[True] > 20 and seen[False] > 20


def test_unknown_kind_or_lattice():
    assert not api.batch_large_supported(L.BONDSITE, 0, 10, 10, 0)
    assert not api.batch_large_supported(-1, 0, 10, 10, 0)
    assert not api.batch_large_supported(L.SITE, 2, 10, 10, 0)
    assert not api.batch_large_supported(L.SITE, 0, 0, 10, 0)
    assert not api.batch_large_supported(L.SITE, 0, 1 << 20, 1 << 20, 0)


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
    assert L.SIGNATURES["perc_batch_large_supported"][1] == L.SIGNATURES["perc_batch_cond_supported"][1]
    import percolation_amd as P
    assert P.batch_large_supported is api.batch_large_supported
    assert hasattr(api.Context, "set_batch_large") and hasattr(api.Ensemble, "set_batch_large")
