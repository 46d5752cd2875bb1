"""The batch kernels' lattices away from square -- TEST INFRASTRUCTURE ONLY,
the helper of test_batch_shapes_host.py and test_batch_shapes.py: the shape
table (which predicate accepts which (lattice, m, n, pbc), per kind) and the
host-side choice of the items a (shape, kind) is run on.

A shape is here for what its size does to a one-workgroup kernel (N = (n - 2)
m interior rows, t = m n sites, 2m electrode entries):

  (0,3,3,0) (0,4,3,1) (1,4,3,1)   the smallest; n = 3: N = m, every system row
                                  touches both electrodes (x_clear / x_add /
                                  x_at's "a row can be both", V() reads no
                                  interior neighbour row, Gtop and Gbot from
                                  the same voltages); pbc with m = 4: the wrap
                                  offsets are as large as the row
  (0,3,4,0)                       two interior rows, each touching one electrode
  (0,3,100,0) (1,4,64,1)          thin: these run to the tolerance
  (0,300,3,0)                     m beyond a workgroup of 256 threads, n = 3
  (0,4096,3,0) (1,2048,3,1)       m >= 4 workgroups, 2m > N (8192 electrode
  (0,2048,4,0)                    entries on 512 threads), N = 4096 or 2048
                                  exactly; the labeling view ends after q
  (0,4500,3,0)                    the bond kind's arena limit: site and mixed
                                  are refused by the default kernel
  (0,64,34,0) | (0,64,35,0)       N = 2048 | 2112: 256 | 512 threads
  (0,64,66,0) | (0,64,67,0)       N = 4096 | 4160: 512 | 1024 threads
  (0,3,2732,0) | (0,3,2733,0)     N = 8190 (one column short of kBatchRows) |
                                  8193 (refused by the default kernel)
  (0,50,71,0) (1,50,51,0)         the weighted kernel's last fits;
  (0,50,72,0) (1,50,52,0)         its first refusals
  (0,256,64,0) (0,1024,16,0)      the large kernel's cap in four aspects: 16
  (0,3,5461,0) (1,4,4096,1)       rows per thread, a ragged last round
  (0,5461,3,0) (0,4096,4,0)       the scan / cluster kernels' cap (t = 16383,
                                  16384) in the flat aspect
  (0,3,5462,0)                    t = 16386: refused by every kernel

The predicates' values below were evaluated on the CPU build of this tree;
test_batch_shapes_host.py holds the library to them.

Items.  Orders: api.shuffled_ids with S = trial_seeds(58302)[0] for the sites
and S + 1 for the bonds.  Fractions f of FRACTIONS; counts int(f t) sites /
int(f nb) bonds, the mixed kind int((0.5 + f / 2) t) sites with int(f nb)
bonds.  select() gives per (shape, kind): `single`, the lowest f at which
exactly one cluster spans; `full`; `spill`, the whole order with its spill
slot (t + 1 / nb + 1); `none`, the highest f at which nothing spans, and
`multi`, the lowest f at which several clusters span, where the grid has
one.  Spanning counts are api.cluster_stats_host's (host only)."""
import collections

from percolation_amd import _lib as L
from percolation_amd import api

B, S, M = L.BOND, L.SITE, L.SITEBOND
KINDS = (B, S, M)
KIND_NAME = {B: "bond", S: "site", M: "mixed"}
ALL, NONE, BOND_ONLY = frozenset(KINDS), frozenset(), frozenset([B])
FRACTIONS = (0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.98, 0.995)
SEED = int(api.trial_seeds(58302, 1)[0])

# cond / large / weighted / currents: the kinds the predicate accepts; scan,
# clusters (at nexact 0, 12 and 1024 alike): bool
Row = collections.namedtuple("Row", "lat cond large weighted currents scan clusters")
TABLE = [
    Row((0, 3, 3, 0), ALL, ALL, ALL, ALL, True, True),
    Row((0, 4, 3, 1), ALL, ALL, ALL, ALL, True, True),
    Row((1, 4, 3, 1), ALL, ALL, ALL, ALL, True, True),
    Row((0, 3, 4, 0), ALL, ALL, ALL, ALL, True, True),
    Row((0, 3, 100, 0), ALL, ALL, ALL, ALL, True, True),
    Row((1, 4, 64, 1), ALL, ALL, ALL, ALL, True, True),
    Row((0, 300, 3, 0), ALL, ALL, ALL, ALL, True, True),
    Row((0, 4096, 3, 0), ALL, ALL, NONE, ALL, True, True),
    Row((1, 2048, 3, 1), ALL, ALL, NONE, ALL, True, True),
    Row((0, 2048, 4, 0), ALL, ALL, NONE, ALL, True, True),
    Row((0, 4500, 3, 0), BOND_ONLY, ALL, NONE, BOND_ONLY, True, True),
    Row((0, 64, 34, 0), ALL, ALL, ALL, ALL, True, True),
    Row((0, 64, 35, 0), ALL, ALL, ALL, ALL, True, True),
    Row((0, 64, 66, 0), ALL, ALL, NONE, ALL, True, True),
    Row((0, 64, 67, 0), ALL, ALL, NONE, ALL, True, True),
    Row((0, 3, 2732, 0), ALL, ALL, NONE, ALL, True, True),
    Row((0, 3, 2733, 0), NONE, ALL, NONE, NONE, True, True),
    Row((0, 50, 71, 0), ALL, ALL, ALL, ALL, True, True),
    Row((1, 50, 51, 0), ALL, ALL, ALL, ALL, True, True),
    Row((0, 50, 72, 0), ALL, ALL, NONE, ALL, True, True),
    Row((1, 50, 52, 0), ALL, ALL, NONE, ALL, True, True),
    Row((0, 256, 64, 0), NONE, ALL, NONE, NONE, True, True),
    Row((0, 1024, 16, 0), NONE, ALL, NONE, NONE, True, True),
    Row((0, 3, 5461, 0), NONE, ALL, NONE, NONE, True, True),
    Row((1, 4, 4096, 1), NONE, ALL, NONE, NONE, True, True),
    Row((0, 5461, 3, 0), NONE, NONE, NONE, NONE, True, True),
    Row((0, 4096, 4, 0), NONE, NONE, NONE, NONE, True, True),
    Row((0, 3, 5462, 0), NONE, NONE, NONE, NONE, False, False),
]
ROW = {r.lat: r for r in TABLE}
assert len(ROW) == len(TABLE)

TINY = [(0, 3, 3, 0), (0, 4, 3, 1), (1, 4, 3, 1), (0, 3, 4, 0)]
THIN = [(0, 3, 100, 0), (1, 4, 64, 1), (0, 3, 2732, 0), (0, 3, 5461, 0), (1, 4, 4096, 1)]
FLAT = [(0, 300, 3, 0), (0, 4096, 3, 0), (1, 2048, 3, 1), (0, 2048, 4, 0), (0, 4500, 3, 0), (0, 1024, 16, 0),
        (0, 5461, 3, 0), (0, 4096, 4, 0)]
# the shapes whose solve would run thousands of iterations: stopped at ITMAX_STOP
LONG = [(0, 3, 2732, 0), (0, 3, 2733, 0), (0, 3, 5461, 0), (1, 4, 4096, 1), (0, 64, 66, 0), (0, 64, 67, 0)]
ITMAX_STOP = 300


def lat_id(lat):
    return "%s%dx%d%s" % ("tri" if lat[0] else "sq", lat[1], lat[2], "p" if lat[3] else "")


def sizes(lat):
    """(N, t, nb)"""
    return (lat[2] - 2) * lat[1], lat[1] * lat[2], api.nbonds(*lat)


def supported(family, lat):
    """the kinds the table gives a family ("cond", "large", "weighted",
    "currents") on a shape"""
    return [k for k in KINDS if k in getattr(ROW[lat], family)]


_ORDERS = {}


def orders(lat):
    """(site order, bond order) of a shape, read-only, formed once"""
    if lat not in _ORDERS:
        _, t, nb = sizes(lat)
        so, bo = api.shuffled_ids(t, SEED), api.shuffled_ids(nb, SEED + 1)
        so.setflags(write=False)
        bo.setflags(write=False)
        _ORDERS[lat] = (so, bo)
    return _ORDERS[lat]


def counts(lat, kind, f):
    """(nsites, nbonds) at fraction f; a list the kind does not read: 0"""
    _, t, nb = sizes(lat)
    if kind == B:
        return 0, int(f * nb)
    if kind == S:
        return int(f * t), 0
    return int((0.5 + f / 2) * t), int(f * nb)


def full_counts(lat, kind, spill=False):
    _, t, nb = sizes(lat)
    e = 1 if spill else 0
    return (t + e if kind != B else 0), (nb + e if kind != S else 0)


def nspan_host(lat, kind, ns, nbc):
    so, bo = orders(lat)
    return int(api.cluster_stats_host(*lat, kind, so, ns, bo, nbc, 0)[0]["nspan"])


_GRID = {}


def grid(lat, kind):
    """[(f, nsites, nbonds, nspan)] over FRACTIONS, ascending, computed once"""
    if (lat, kind) not in _GRID:
        _GRID[lat, kind] = [(f,) + counts(lat, kind, f) + (nspan_host(lat, kind, *counts(lat, kind, f)),)
                            for f in FRACTIONS]
    return _GRID[lat, kind]


def select(lat, kind):
    """dict name -> (nsites, nbonds): single, full, spill always; none and
    multi where the grid has one.  KeyError "single" never: the host test
    holds every supported (shape, kind) to a partial single-spanning item."""
    g = grid(lat, kind)
    out = {}
    once = [x for x in g if x[3] == 1]
    if once:
        out["single"] = once[0][1:3]
    out["full"] = full_counts(lat, kind)
    out["spill"] = full_counts(lat, kind, spill=True)
    zero = [x for x in g if x[3] == 0]
    if zero:
        out["none"] = zero[-1][1:3]
    many = [x for x in g if x[3] > 1]
    if many:
        out["multi"] = many[0][1:3]
    return out


def batch_kw(lat, kind, items):
    """Context.batch_cond's / batch_clusters' order and count arguments for a
    list of (nsites, nbonds) items of the shape's one trial"""
    so, bo = orders(lat)
    kw = {}
    if kind != B:
        kw.update(site_orders=so, item_nsites=[x[0] for x in items])
    if kind != S:
        kw.update(bond_orders=bo, item_nbonds=[x[1] for x in items])
    return kw
