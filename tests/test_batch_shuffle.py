"""The device shuffle (perc_batch_shuffle, k_shuffle_ranks) and the seeded
batch entry points (perc_batch_scan_seeded, perc_batch_cond_seeded):

* orders and ranks entry for entry the host's (perc_shuffle_seeded and the
  ranks its order implies) on list lengths around the wave width, the batch
  paths' own lists, the 128 x 128 bond list and the longest supported list;
  ordinary, degenerate and negative seeds, and seeds whose shuffle reaches
  the spill slot (asserted on the host order);
* seeded scans record for record the order-taking scans of the same seeds;
  the bond_perc / site_perc / sb_perc goldens through device_shuffle=True and
  the Fortran drivers' dshuffle key, byte for byte;
* cond_curve(device_shuffle=True) bitwise the host-shuffle curve; a seeded
  batch_cond whose order-taking twin reports fallback items;
* ntrials 0 and 1, one seed at both ends of a 200-trial call, the context's
  single-realisation state left alone, repeatability, the argument errors."""
import numpy as np
import pytest

import golden_io as G
import test_fortran_drivers as F
from percolation_amd import _lib as L
from percolation_amd import api

pytestmark = pytest.mark.gpu
PERC = [v for v in G.variants() if G.meta(v)["kind"] in ("bond_perc", "site_perc")]
SB = [v for v in G.variants() if G.meta(v)["kind"] == "sb_perc"]
CAP = [(0, 128, 128, 0), (1, 128, 128, 0)]
N_MAX = 65534  # the longest list perc_shuffle_device_supported accepts

# degenerate and edge seeds: 0 is 123459876; 2147483647 sticks the recurrence
# at 0 (every target clamps to N + 1); a negative seed wraps as unsigned 64 bit
EDGE_SEEDS = [0, 1, 2147483646, 2147483647, -5]
# seeds whose shuffle swaps with the spill slot, by list length
SPILL = {180: [44401, 129473], 100: [128343], 2500: [1033], 4900: [1872]}


def trial_seeds8():
    return [int(s) for s in api.trial_seeds(58302, 8, scale=1000000)]


def host_order(N, seed):
    a = np.zeros(N + 1, dtype=np.int32)
    L.lib().perc_shuffle_seeded(int(seed), N, a)
    return a


def implied_ranks(order):
    N = len(order) - 1
    r = np.full(N, -1, dtype=np.int32)
    pos = np.arange(N + 1, dtype=np.int32)
    el = order != 0
    r[order[el] - 1] = pos[el]
    assert (r >= 0).all()
    return r


def check_shuffle(ctx, seeds, N, **kw):
    o, r = ctx.batch_shuffle(seeds=np.array(seeds, np.int32), orders=True, ranks=True, **kw)
    assert o.shape == (len(seeds), N + 1) and r.shape == (len(seeds), N)
    for k, s in enumerate(seeds):
        want = host_order(N, s)
        assert np.array_equal(o[k], want), (N, s, np.flatnonzero(o[k] != want)[:8])
        assert np.array_equal(r[k], implied_ranks(want)), (N, s)


@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 100, 180, 2500, 4900])
def test_orders_and_ranks_bitwise(N):
    seeds = trial_seeds8() + EDGE_SEEDS + SPILL.get(N, [])
    for s in SPILL.get(N, []):  # a wrong seed must fail, not test nothing
        assert host_order(N, s)[N] != 0, (N, s)
    with api.Context(0, 10, 10, 0) as ctx:
        check_shuffle(ctx, seeds, N, list=None, n=N)


@pytest.mark.parametrize("lat", [(0, 10, 10, 0), (0, 50, 50, 0)])
def test_lattice_lists_bitwise(lat):
    """the same through list BOND / SITE: N = 180 / 100 and 4900 / 2500"""
    with api.Context(*lat) as ctx:
        for lst, N in ((L.BOND, ctx.nb), (L.SITE, ctx.t)):
            seeds = trial_seeds8() + EDGE_SEEDS + SPILL[N]
            check_shuffle(ctx, seeds, N, list=lst)


def test_square_128_bond_list():
    with api.Context(0, 128, 128, 0) as ctx:
        assert ctx.nb == 32512
        check_shuffle(ctx, trial_seeds8()[:2], ctx.nb, list=L.BOND)


def test_longest_list():
    assert api.shuffle_device_supported(N_MAX) and not api.shuffle_device_supported(N_MAX + 1)
    with api.Context(0, 10, 10, 0) as ctx:
        check_shuffle(ctx, trial_seeds8()[:1], N_MAX, list=None, n=N_MAX)


# ---------------------------------------------------------------- scans
def host_orders(N, seeds):
    return np.stack([host_order(N, s) for s in seeds])


@pytest.mark.parametrize("kind", [L.BOND, L.SITE])
@pytest.mark.parametrize("lat", [(0, 10, 10, 0), (0, 10, 10, 1), (1, 12, 9, 1), (0, 5, 3, 0), (0, 50, 50, 0),
                                 (1, 50, 50, 0)])
def test_seeded_scan_equals_order_scan(lat, kind):
    seeds = np.array(trial_seeds8(), np.int32)
    with api.Context(*lat) as ctx:
        N = ctx.nb if kind == L.BOND else ctx.t
        name = "bond" if kind == L.BOND else "site"
        want = ctx.batch_scan(kind, **{name + "_orders": host_orders(N, seeds)})
        got = ctx.batch_scan_seeded(kind, **{name + "_seeds": seeds})
    assert got == want and len(got) == 8
    assert any(g["first"] > 0 for g in got)


@pytest.mark.parametrize("scan", [L.BOND, L.SITE])
def test_seeded_mixed_scan(scan):
    lat = (1, 20, 16, 1)
    ss, bs = np.arange(1, 9, dtype=np.int32), np.arange(78, 86, dtype=np.int32)
    with api.Context(*lat) as ctx:
        fixed = int(0.8 * ctx.t) if scan == L.BOND else int(0.6 * ctx.nb)
        want = ctx.batch_scan(L.SITEBOND, site_orders=host_orders(ctx.t, ss),
                              bond_orders=host_orders(ctx.nb, bs), scan=scan, fixed=fixed)
        got = ctx.batch_scan_seeded(L.SITEBOND, site_seeds=ss, bond_seeds=bs, scan=scan, fixed=fixed)
    assert got == want and len(got) == 8
    assert any(g["first"] > 0 for g in got)


@pytest.mark.parametrize("kind", [L.BOND, L.SITE])
@pytest.mark.parametrize("lat", CAP)
def test_seeded_scan_size_cap(lat, kind):
    seed = np.array(trial_seeds8()[:1], np.int32)
    with api.Context(*lat) as ctx:
        N = ctx.nb if kind == L.BOND else ctx.t
        name = "bond" if kind == L.BOND else "site"
        want = ctx.batch_scan(kind, **{name + "_orders": host_orders(N, seed)})
        got = ctx.batch_scan_seeded(kind, **{name + "_seeds": seed})
    assert got == want and got[0]["first"] > 0


# ---------------------------------------------------------------- goldens
@pytest.fixture
def no_host_shuffle(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("shuffled_ids called on the device-shuffle path")
    monkeypatch.setattr(api, "shuffled_ids", refuse)


@pytest.mark.parametrize("v", PERC)
def test_threshold_scan_goldens(v, no_host_shuffle):
    md = G.meta(v)
    p = md["params"]
    kind = L.BOND if md["kind"] == "bond_perc" else L.SITE
    rows = api.threshold_scan(p["lattice"], p["m"], p["n"], p["pbc"], kind, p["seed"], p["numtrials"],
                              batch=16, device_shuffle=True)
    assert api.fmt_perc_rows(rows).encode() == G.text(v, md["kind"] + ".txt")


@pytest.mark.parametrize("v", SB)
def test_sb_perc_goldens(v, no_host_shuffle):
    p = G.meta(v)["params"]
    rows = api.mixed_scan(p["lattice"], p["m"], p["n"], p["pbc"], L.BOND, p["seed"], p["points"],
                          p["iters"], batch=16, device_shuffle=True)
    assert api.fmt_mixed_rows(rows).encode() == G.text(v, "sb_perc.txt")


@pytest.mark.parametrize("v", ["sq_bond_perc", "tri_site_perc", "sq_sb_perc"])
def test_fortran_dshuffle_key(v, tmp_path):
    md, r = F.run_variant(v, tmp_path, extra=("batch=16", "dshuffle=1"))
    name = md["kind"] + ".txt"
    assert (tmp_path / name).read_bytes() == G.text(v, name)
    assert len(r.stdout.splitlines()) == len(G.text(v, name).splitlines())


def test_device_shuffle_ignored_without_batch():
    kw = dict(lattice=0, m=10, n=10, pbc=0, kind=L.BOND, master=58302, numtrials=3)
    assert api.threshold_scan(device_shuffle=True, **kw) == api.threshold_scan(**kw)


# ---------------------------------------------------------------- conductance
@pytest.mark.parametrize("literal", [False, True], ids=["fast", "literal"])
@pytest.mark.parametrize("L_", [10, 50])
@pytest.mark.parametrize("kind", [L.SITE, L.SITEBOND], ids=["site", "mixed"])
def test_cond_curve_bitwise(kind, L_, literal):
    """same kernel, same ranks, same accumulation order: the same bits"""
    grid = (0.6, 0.7, 1.0) if kind == L.SITE else ((0.7, 0.8), (0.9, 0.9), (1.0, 1.0))
    with api.Context(0, L_, L_, 0) as ctx:
        if literal:
            ctx.set_dot_order(L.DOT_LITERAL)
        kw = dict(lattice=0, m=L_, n=L_, pbc=0, kind=kind, grid=grid, numtrials=3, ctx=ctx)
        off_t, off_s = api.cond_curve(device_shuffle=False, **kw)
        on_t, on_s = api.cond_curve(device_shuffle=True, **kw)
    assert repr(on_t) == repr(off_t) and len(on_t) == 3
    assert on_s.tobytes() == off_s.tobytes()
    assert any(r["spanning"] for t in on_t for r in t["rows"])


@pytest.mark.parametrize("kind", [L.SITE, L.SITEBOND], ids=["site", "mixed"])
def test_seeded_batch_cond_with_fallback_items(kind):
    """a wide, short lattice: several clusters span at moderate fractions, so
    the order-taking call replays some items through the single path; the
    seeded call regenerates those trials' orders on the host -- equal items"""
    lat = (0, 48, 4, 0)
    ss, bs = np.arange(11, 15, dtype=np.int32), np.arange(91, 95, dtype=np.int32)
    fr = (0.55, 0.65, 0.75, 0.85) if kind == L.SITE else (0.8, 0.85, 0.9, 0.95)
    with api.Context(*lat) as ctx:
        assert api.batch_cond_supported(kind, *lat)
        it = np.repeat(np.arange(4, dtype=np.int32), len(fr))
        ns = np.tile(np.array([int(f * ctx.t) for f in fr], np.int32), 4)
        nbc = np.tile(np.array([int(f * ctx.nb) for f in fr], np.int32), 4) if kind == L.SITEBOND else None
        kw = dict(item_nsites=ns, item_nbonds=nbc, tol=1e-10, itmax=5000)
        bo = host_orders(ctx.nb, bs) if kind == L.SITEBOND else None
        want = ctx.batch_cond(kind, it, site_orders=host_orders(ctx.t, ss), bond_orders=bo, **kw)
        nfall = sum(w["fallback"] for w in want)
        print("fallback items on the order-taking call: %d of %d" % (nfall, len(want)))
        assert nfall >= 1
        got = ctx.batch_cond(kind, it, site_seeds=ss, bond_seeds=bs if kind == L.SITEBOND else None, **kw)
    assert repr(got) == repr(want)


# ---------------------------------------------------------------- mechanics
def test_mechanics():
    with api.Context(0, 10, 10, 0) as ctx:
        nb = ctx.nb
        seeds = np.arange(1000, 1200, dtype=np.int32)
        seeds[199] = seeds[0]
        want = ctx.batch_scan(L.BOND, bond_orders=host_orders(nb, seeds))
        # a previously occupied context keeps its state over a seeded call
        ctx.occupy(L.BOND, bond_order=host_order(nb, 1005), nbonds_=int(0.6 * nb))
        before = ctx.label()
        got = ctx.batch_scan_seeded(L.BOND, bond_seeds=seeds)
        assert ctx.label() == before
        assert got == want and got[0] == got[199]
        assert ctx.batch_scan_seeded(L.BOND, bond_seeds=seeds) == got  # two identical calls
        assert ctx.batch_scan_seeded(L.BOND, bond_seeds=seeds[:0]) == []
        assert ctx.batch_scan_seeded(L.BOND, bond_seeds=seeds[:1]) == got[:1]
        o0, r0 = ctx.batch_shuffle(L.BOND, seeds[:0], orders=True, ranks=True)
        assert o0.shape == (0, nb + 1) and r0.shape == (0, nb)
        o1, r1 = ctx.batch_shuffle(L.SITE, seeds[:1], orders=True, ranks=True)
        o2, r2 = ctx.batch_shuffle(L.SITE, seeds[:1], orders=True, ranks=True)
        assert np.array_equal(o1, o2) and np.array_equal(r1, r2)
        assert np.array_equal(o1[0], host_order(ctx.t, seeds[0]))
        assert ctx.batch_shuffle(L.SITE, seeds[:3]) == (None, None)
        it = np.zeros(0, np.int32)
        assert ctx.batch_cond(L.SITE, it, site_seeds=seeds[:2], item_nsites=it) == []


def test_errors_are_einval():
    einval = pytest.raises(L.PercError, match="PERC_EINVAL")
    lib = L.lib()
    sd = np.arange(1, 4, dtype=np.int32)
    with api.Context(0, 200, 200, 0) as ctx:  # nb = 79600: past the 16-bit entries
        assert not api.shuffle_device_supported(ctx.nb) and api.shuffle_device_supported(ctx.t)
        with einval:
            ctx.batch_shuffle(L.BOND, sd)
        with einval:
            ctx.batch_scan_seeded(L.BOND, bond_seeds=sd)
    with api.Context(0, 10, 10, 0) as ctx:
        for n in (0, -1, N_MAX + 1):
            with einval:
                ctx.batch_shuffle(None, sd, n=n)
        with einval:
            ctx.batch_shuffle(7, sd)
        with einval:
            ctx.batch_shuffle(L.SITEBOND, sd)
        for kw in (dict(kind=L.BONDSITE, site_seeds=sd, bond_seeds=sd, fixed=5),
                   dict(kind=L.SITEBOND, site_seeds=sd, bond_seeds=sd, scan=3, fixed=5),
                   dict(kind=L.SITEBOND, site_seeds=sd, bond_seeds=sd),
                   dict(kind=L.SITEBOND, site_seeds=sd, bond_seeds=sd, scan=L.BOND, fixed=ctx.t + 1),
                   dict(kind=L.BOND, site_seeds=sd),
                   dict(kind=L.SITE, bond_seeds=sd),
                   dict(kind=L.SITEBOND, site_seeds=sd, fixed=5)):
            with einval:
                ctx.batch_scan_seeded(**kw)
        it = np.zeros(3, np.int32)
        cnt = np.full(3, 50, np.int32)
        for kw in (dict(kind=L.SITE, bond_seeds=sd, item_nsites=cnt),
                   dict(kind=L.SITEBOND, site_seeds=sd, item_nsites=cnt, item_nbonds=cnt),
                   dict(kind=L.BONDSITE, site_seeds=sd, bond_seeds=sd, item_nsites=cnt, item_nbonds=cnt),
                   dict(kind=L.SITE, site_seeds=sd, item_nsites=cnt, rule=L.RULE_BOND)):
            with einval:
                ctx.batch_cond(item_trial=it, **kw)
        out = (L.ScanItem * 4)()
        assert lib.perc_batch_shuffle(ctx.h, L.BOND, -1, L.ptr(sd), None, None) == -1
        assert lib.perc_batch_shuffle(ctx.h, L.BOND, 3, None, None, None) == -1
        assert "seeds" in lib.perc_last_error().decode()
        assert lib.perc_batch_shuffle(ctx.h, L.BOND, 0, None, None, None) == 0
        assert lib.perc_batch_scan_seeded(ctx.h, L.BOND, L.BOND, -1, None, L.ptr(sd), None, out) == -1
        assert lib.perc_batch_scan_seeded(ctx.h, L.BOND, L.BOND, 0, None, None, None, None) == 0
        assert lib.perc_batch_cond_seeded(ctx.h, L.SITE, L.RULE_SITE, L.CUR_MATLAB, -1, L.ptr(sd), None, 0,
                                          None, None, None, 1, 1.0, 1.0, 1e-12, 2, 1e-8, 100, None) == -1
        assert lib.perc_batch_cond_seeded(ctx.h, L.SITE, L.RULE_SITE, L.CUR_MATLAB, 0, None, None, 0,
                                          None, None, None, 1, 1.0, 1.0, 1e-12, 2, 1e-8, 100, None) == 0
