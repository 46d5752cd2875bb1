"""The context's one rank store (perc_batch.h): every batch call -- conductance
in all its forms, scans, cluster tables, from orders or from seeds -- forms its
launches' rank arrays in the same device buffers, numbered per run.  Whatever
ran before on a context, a call gives what it gives on a fresh one, bit for
bit (the literal dot order: the solves are reproducible to the bit):

* nine calls of every path, orders and seeds alternating, on one context;
* 64 trials, then 3, then 65: the buffers grown, reused larger than needed,
  grown again;
* items that name two of six trials against the same items on a call of those
  two trials alone: a run holds the trials it names, renumbered.

The ensemble's sequence over one filling of the store (batch_upload_orders,
batch_run_items, batch_scan_uploaded, batch_run_items) is test_batch.py's
Ensemble(batch=...) cases: their lattices lie within the scan kernel's."""
import numpy as np
import pytest

from percolation_amd import _lib as L
from percolation_amd import api

pytestmark = pytest.mark.gpu
LATTICES = [(0, 10, 10, 0), (1, 8, 6, 0)]  # square; triangular, m even
KINDS = [L.BOND, L.SITE, L.SITEBOND]
NTRIALS = 6
ITEM_TRIAL = np.array([4, 1, 3, 1, 0, 5, 3, 4], np.int32)  # out of order, repeats, trial 2 never named
FRACTIONS = [0.45, 0.58, 0.64, 0.7, 0.76, 0.85, 1.0, None]  # None: the whole order, spill slot included


def same(a, b):
    """bitwise equality of two results: records, lists of dicts, arrays, floats"""
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return a == b


_INPUTS = {}


def inputs(lat, ntrials=NTRIALS):
    """orders, seeds and the item counts of a lattice (made once, read-only)"""
    key = (lat, ntrials)
    if key not in _INPUTS:
        t, nb = lat[1] * lat[2], api.nbonds(*lat)
        sseed = np.arange(ntrials, dtype=np.int32) * 7919 + 143285
        bseed = np.arange(ntrials, dtype=np.int32) * 104729 + 43716
        so = np.stack([api.shuffled_ids(t, int(s)) for s in sseed])
        bo = np.stack([api.shuffled_ids(nb, int(s)) for s in bseed])
        ns = np.array([t + 1 if f is None else round(f * t) for f in FRACTIONS], np.int32)
        nbc = np.array([nb + 1 if f is None else round(f * nb) for f in FRACTIONS], np.int32)
        for a in (sseed, bseed, so, bo, ns, nbc):
            a.setflags(write=False)
        _INPUTS[key] = dict(sseed=sseed, bseed=bseed, so=so, bo=bo, ns=ns, nbc=nbc)
    return _INPUTS[key]


def lists(kind, d, seeded, it=ITEM_TRIAL, rows=None):
    """the keyword arguments of an item call of a kind: its order or seed lists
    (rows: those trials only) and its count lists"""
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    kw = {}
    if kind != L.BOND:
        kw["item_nsites"] = d["ns"][:len(it)]
        kw["site_seeds" if seeded else "site_orders"] = pick(d["sseed"] if seeded else d["so"])
    if kind != L.SITE:
        kw["item_nbonds"] = d["nbc"][:len(it)]
        kw["bond_seeds" if seeded else "bond_orders"] = pick(d["bseed"] if seeded else d["bo"])
    return kw


def scan_lists(kind, d, seeded):
    kw = {k: v for k, v in lists(kind, d, seeded).items() if not k.startswith("item_")}
    if kind == L.SITEBOND:
        kw["fixed"] = int(d["ns"][5])
    return kw


def calls(lat):
    """(name, call) of the sequence: every path, orders and seeds alternating"""
    d = inputs(lat)
    it = ITEM_TRIAL
    wseed = np.arange(len(it)) * 31 + 1838534
    seq = []
    for kind in KINDS:
        seq.append(("cond orders %d" % kind, lambda c, k=kind: c.batch_cond(k, it, **lists(k, d, False))))
    for kind in KINDS:
        seq.append(("scan orders %d" % kind, lambda c, k=kind: c.batch_scan(k, **scan_lists(k, d, False))))
    for kind in KINDS:
        seq.append(("clusters seeded %d" % kind,
                    lambda c, k=kind: c.batch_clusters(k, it, nexact=16, **lists(k, d, True))))
    for kind in KINDS:
        seq.append(("cond seeded %d" % kind, lambda c, k=kind: c.batch_cond(k, it, **lists(k, d, True))))
    for kind in KINDS:
        seq.append(("scan seeded %d" % kind, lambda c, k=kind: c.batch_scan_seeded(k, **scan_lists(k, d, True))))
    for kind in KINDS:
        seq.append(("clusters orders %d" % kind,
                    lambda c, k=kind: c.batch_clusters(k, it, nexact=16, **lists(k, d, False))))
    for kind in KINDS:
        seq.append(("cond wseed %d" % kind,
                    lambda c, k=kind: c.batch_cond(k, it, item_wseed=wseed, **lists(k, d, False))))
    for kind in KINDS:
        seq.append(("cond currents %d" % kind,
                    lambda c, k=kind: c.batch_cond(k, it, currents=True, voltages=True, **lists(k, d, False))))
    seq.append(("bondc", lambda c: c.batch_bondc(d["bo"], it, d["nbc"])))
    return seq


def fresh(lat, call):
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        return call(ctx)


@pytest.mark.parametrize("lat", LATTICES)
def test_one_store_many_users(lat):
    for kind in KINDS:
        assert api.batch_cond_supported(kind, *lat) and api.batch_weighted_supported(kind, *lat)
    assert api.scan_supported(*lat) and api.batch_clusters_supported(*lat, 16)
    seq = calls(lat)
    want = [fresh(lat, call) for _, call in seq]
    # the sequence solves something: the comparison below is not of empty records
    assert any(o["nspan"] > 0 and o["iter"] > 0 and o["gtop"] > 0.0 for o in want[0])
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        for (name, call), w in zip(seq, want):
            assert same(call(ctx), w), (lat, name)
        for (name, call), w in reversed(list(zip(seq, want))):  # ... and every path after its successor
            assert same(call(ctx), w), (lat, name, "reversed")


@pytest.mark.parametrize("lat", LATTICES)
def test_grow_and_shrink(lat):
    def run(ctx, ntrials):
        d = inputs(lat, ntrials)
        it = np.arange(ntrials, dtype=np.int32)[::-1].copy()
        cnt = dict(item_nsites=np.resize(d["ns"], ntrials), item_nbonds=np.resize(d["nbc"], ntrials))
        return [ctx.batch_cond(L.SITEBOND, it, site_orders=d["so"], bond_orders=d["bo"], **cnt),
                ctx.batch_scan(L.BOND, bond_orders=d["bo"]),
                ctx.batch_clusters(L.SITE, it, site_seeds=d["sseed"], item_nsites=cnt["item_nsites"], nexact=16),
                ctx.batch_cond(L.SITE, it, site_seeds=d["sseed"], item_nsites=cnt["item_nsites"]),
                ctx.batch_scan_seeded(L.SITE, site_seeds=d["sseed"])]

    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        for ntrials in (64, 3, 65):
            assert same(run(ctx, ntrials), fresh(lat, lambda c: run(c, ntrials))), (lat, ntrials)


@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("lat", LATTICES)
def test_unnamed_and_renumbered_trials(lat, seeded):
    d = inputs(lat)
    it = np.array([5, 2, 2, 5, 5, 2, 5, 2], np.int32)
    rows = np.array([5, 2])
    remap = np.where(it == 5, 0, 1).astype(np.int32)
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        for kind in KINDS:
            six = ctx.batch_cond(kind, it, **lists(kind, d, seeded, it))
            two = ctx.batch_cond(kind, remap, **lists(kind, d, seeded, it, rows))
            assert same(six, two), (lat, kind, "cond")
            assert any(o["nspan"] > 0 for o in six)
            six = ctx.batch_clusters(kind, it, nexact=16, **lists(kind, d, seeded, it))
            two = ctx.batch_clusters(kind, remap, nexact=16, **lists(kind, d, seeded, it, rows))
            assert same(six, two), (lat, kind, "clusters")
        if not seeded:
            six = ctx.batch_cond(L.BOND, it, currents=True, voltages=True, **lists(L.BOND, d, False, it))
            two = ctx.batch_cond(L.BOND, remap, currents=True, voltages=True, **lists(L.BOND, d, False, it, rows))
            assert same(six, two), (lat, "currents")
