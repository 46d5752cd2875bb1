"""perc_scan_supported (host-only): which lattices the scan kernel takes --
up to 16384 sites (128 x 128) on both lattices, with and without pbc -- the
`batch` keyword of the scan mirrors, and the symbols of the batched scans in
libperc.so.  No device."""
import inspect

import pytest

from percolation_amd import _lib as L
from percolation_amd import api


@pytest.mark.parametrize("lattice,m,n,pbc,want", [
    (0, 128, 128, 0, True), (1, 128, 128, 1, True), (0, 50, 50, 0, True), (1, 5, 3, 0, True),
    (0, 129, 128, 0, False), (1, 128, 129, 0, False),
])
def test_scan_supported(lattice, m, n, pbc, want):
    assert L.lib().perc_scan_supported(lattice, m, n, pbc) == (1 if want else 0)
    assert api.scan_supported(lattice, m, n, pbc) is want


@pytest.mark.parametrize("fn", [api.threshold_scan, api.mixed_scan])
def test_scans_accept_batch(fn):
    p = inspect.signature(fn).parameters
    assert "batch" in p and p["batch"].default == 0


def test_batch_scan_signature():
    p = inspect.signature(api.Context.batch_scan).parameters
    assert list(p)[1:] == ["kind", "site_orders", "bond_orders", "scan", "fixed"]
    assert p["scan"].default == L.BOND and p["fixed"].default is None


def test_scan_symbols_declared():
    lib = L.lib()
    for name in ("perc_batch_scan", "perc_scan_supported"):
        assert name in L.SIGNATURES
        assert getattr(lib, name) is not None
