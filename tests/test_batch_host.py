"""perc_batch_supported (host-only): which lattices the batch kernel takes --
n >= 3, (n-2)*m <= 8192 interior rows, the stencil operator exists."""
import pytest

from percolation_amd import _lib as L
from percolation_amd import api

CASES = [
    (L.SQUARE, 10, 10, 0, True),
    (L.SQUARE, 50, 50, 0, True),
    (L.SQUARE, 64, 130, 0, True),    # N = 8192, the cap
    (L.SQUARE, 90, 93, 0, True),     # N = 8190
    (L.SQUARE, 91, 93, 0, False),    # N = 8281
    (L.SQUARE, 128, 128, 0, False),
    (L.SQUARE, 10, 2, 0, False),     # n < 3
    (L.TRIANGULAR, 10, 10, 0, True),
]


@pytest.mark.parametrize("lattice,m,n,pbc,want", CASES)
def test_batch_supported(lattice, m, n, pbc, want):
    assert L.lib().perc_batch_supported(lattice, m, n, pbc) == (1 if want else 0)
    assert api.batch_supported(lattice, m, n, pbc) is want


def test_batch_symbols_declared():
    """the batch entry points are in the library with the header's signatures"""
    lib = L.lib()
    for name in ("perc_batch_supported", "perc_batch_bondc", "perc_ensemble_set_batch",
                 "perc_ensemble_batch"):
        assert name in L.SIGNATURES and hasattr(lib, name)
