"""perc_batch_cond_supported (host-only): which lattices the batch kernel
takes per kind -- perc_batch_supported for the bond kind; for the site and
mixed kinds the same checks with the kind's own LDS layout (one more byte per
site in the labeling view)."""
import itertools

import pytest

from percolation_amd import _lib as L
from percolation_amd import api

SIZES = (3, 10, 50, 64, 90, 91, 130)
KINDS = (L.SITE, L.SITEBOND)
# the lattices of tests/test_batch_cond.py
GPU_LATTICES = [(0, 10, 10, 0), (0, 10, 10, 1), (1, 10, 10, 0), (1, 12, 10, 1), (0, 50, 50, 0), (0, 64, 130, 0),
                (0, 90, 93, 0), (1, 64, 130, 1), (0, 8, 8, 0), (1, 48, 48, 1)]


def sweep():
    return itertools.product((L.SQUARE, L.TRIANGULAR), SIZES, SIZES, (0, 1))


def test_bond_kind_is_batch_supported():
    seen = set()
    for lattice, m, n, pbc in sweep():
        want = api.batch_supported(lattice, m, n, pbc)
        assert api.batch_cond_supported(L.BOND, lattice, m, n, pbc) is want, (lattice, m, n, pbc)
        assert L.lib().perc_batch_cond_supported(L.BOND, lattice, m, n, pbc) == (1 if want else 0)
        seen.add(want)
    assert seen == {True, False}


@pytest.mark.parametrize("kind", KINDS)
def test_false_where_batch_supported_is_false(kind):
    for lattice, m, n, pbc in sweep():
        if not api.batch_supported(lattice, m, n, pbc):
            assert not api.batch_cond_supported(kind, lattice, m, n, pbc), (lattice, m, n, pbc)
    assert not api.batch_cond_supported(kind, 0, 91, 93, 0)   # N = 8281
    assert not api.batch_cond_supported(kind, 0, 128, 128, 0)
    assert not api.batch_cond_supported(kind, 0, 10, 2, 0)    # n < 3


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lat", [(0, 64, 130, 0), (0, 90, 93, 0), (1, 64, 130, 1)] + GPU_LATTICES)
def test_true_on_the_tested_lattices(kind, lat):
    assert api.batch_supported(*lat)
    assert api.batch_cond_supported(kind, *lat) is True


def test_unknown_kind_or_lattice():
    assert not api.batch_cond_supported(L.BONDSITE, 0, 10, 10, 0)
    assert not api.batch_cond_supported(-1, 0, 10, 10, 0)
    assert not api.batch_cond_supported(L.SITE, 2, 10, 10, 0)
    assert not api.batch_cond_supported(L.SITE, 0, 0, 10, 0)


def test_symbols_declared():
    """the entry points are in the library with the header's signatures"""
    lib = L.lib()
    for name in ("perc_batch_cond_supported", "perc_batch_cond"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert api.natural_cur_rule(L.BOND) == L.CUR_FORTRAN
    assert api.natural_cur_rule(L.SITE) == api.natural_cur_rule(L.SITEBOND) == L.CUR_MATLAB
