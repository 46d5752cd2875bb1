"""The device shuffle's host-only side (no GPU): the symbols are exported and
perc_shuffle_device_supported accepts every list the batch paths can ask for
-- the bond and site lists of test_batch_scan.py's lattices and of the
triangular 128 x 128 pbc lattice, the longest -- and nothing past the 16-bit
cap of the LDS entries."""
from percolation_amd import _lib as L
from percolation_amd import api

# test_batch_scan.py's LATTICES and CAP (that module is GPU-marked as a whole)
LATTICES = [(0, 10, 10, 0), (0, 10, 10, 1), (1, 10, 10, 0), (1, 12, 9, 1), (0, 5, 3, 0), (0, 37, 23, 0),
            (0, 50, 50, 0), (1, 50, 50, 0)]
CAP = [(0, 128, 128, 0), (1, 128, 128, 0)]
LONGEST = (1, 128, 128, 1)
N_CAP = 65534  # N + 1 <= 65535 (include/perc.h)


def test_symbols_exported():
    lib = L.lib()
    for name in ("perc_shuffle_device_supported", "perc_batch_shuffle", "perc_batch_scan_seeded",
                 "perc_batch_cond_seeded"):
        assert name in L.SIGNATURES
        assert getattr(lib, name) is not None


def test_supported_range():
    f = L.lib().perc_shuffle_device_supported
    for n in (0, -1, -65534, -(1 << 31)):
        assert f(n) == 0, n
    assert f(1) == 1 and f(N_CAP) == 1
    for n in (N_CAP + 1, N_CAP + 2, 1 << 16, 1 << 20, (1 << 31) - 1):
        assert f(n) == 0, n
    assert api.shuffle_device_supported(1) is True and api.shuffle_device_supported(0) is False


def test_every_batch_list_supported():
    for lat in LATTICES + CAP + [LONGEST]:
        assert api.scan_supported(*lat), lat
        t, nb = lat[1] * lat[2], api.nbonds(*lat)
        assert api.shuffle_device_supported(t), (lat, t)
        assert api.shuffle_device_supported(nb), (lat, nb)
    assert api.nbonds(*LONGEST) == max(api.nbonds(lat, 128, 128, pbc) for lat in (0, 1) for pbc in (0, 1))
