"""The batch path (perc_batch_bondc, k_batch_bondc): many small bond
realisations in one launch, one workgroup each, checked against the single
path (perc_occupy / perc_label / perc_conductance) item by item:

* labels and the three outcomes (nothing spans, one cluster, several ->
  fallback) on every pb_grid count of three trials;
* the literal dot order bitwise (conductances, iterations, err), the
  bond_cond goldens through Ensemble(batch=64);
* the fast order: deterministic, independent of the item's place in the
  grid, as accurate as the project asks of a re-associated solve
  (test_config_goldens.py: 2 trunc + max(1e-10, tol));
* non-unit Va, g0 and leak, the leak on both sides of the 1e-10 threshold of
  the currents: the literal order bitwise the single path and the oracle;
* the size cap (N = 8192), a ragged last thread row (N = 8190), the H2 spill
  slot, a forced two-cluster fallback, the ensemble switch and the Fortran
  driver's `batch` key.

The single-path reference of a lattice is computed once and shared."""
import os
import subprocess

import numpy as np
import pytest

import golden_io as G
import oracle_lib as O
import rule_systems as R
from percolation_amd import _lib as L
from percolation_amd import api

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "percolation_amd", "fortran", "bin")
BOND_COND = ["sq_bond_cond", "sq_bond_cond_3t", "tri_bond_cond"]
TOL, ITMAX = 1e-8, 2500
TIGHT, TIGHT_ITMAX = 1e-13, 20000
LATTICES = [(0, 10, 10, 0), (0, 10, 10, 1), (1, 10, 10, 0), (0, 50, 50, 0)]
LABEL_KEYS = ("nclusters", "nspan", "span_root", "span_sites")
COND_KEYS = ("gtop", "gbot", "iter", "err", "status")


def single(ctx, order, count, solve=True, tol=TOL, itmax=ITMAX):
    """the single path on the first `count` entries of `order` (nb + 1: the
    whole order, the spill slot dropped)"""
    o, n = order, count
    if count > ctx.nb:
        o = np.ascontiguousarray(order[order != 0])
        n = len(o)
    ctx.occupy(L.BOND, bond_order=o, nbonds_=int(n))
    li = ctx.label()
    c = ctx.conductance(L.RULE_BOND, L.CUR_FORTRAN, 1.0, 1.0, api.LEAK, 2, tol, itmax) if solve else None
    return li, c


_REF = {}


def reference(lat):
    """trials 0..2 of trial_seeds(58302), every pb_grid count plus 0, 1, nb
    and nb + 1: orders, items and the single path's labels and literal
    conductances (tol 1e-8, itmax 2500), computed once per lattice"""
    if lat in _REF:
        return _REF[lat]
    lattice, m, n, pbc = lat
    seeds = api.trial_seeds(58302, 3)
    with api.Context(lattice, m, n, pbc) as ctx:
        nb = ctx.nb
        ctx.set_dot_order(L.DOT_LITERAL)
        counts = sorted({int(c) for c in api.pb_grid(lattice, nb) if 0 < c <= nb} | {0, 1, nb, nb + 1})
        orders = np.stack([api.shuffled_ids(nb, int(s)) for s in seeds])
        it = [(tr, c) for tr in range(3) for c in counts]
        lab, cond = [], []
        for tr, c in it:
            li, cr = single(ctx, orders[tr], c)
            lab.append(li)
            cond.append(cr)
    _REF[lat] = dict(orders=orders, trial=np.array([x[0] for x in it], np.int32),
                     count=np.array([x[1] for x in it], np.int32), label=lab, cond=cond, nb=nb)
    return _REF[lat]


@pytest.mark.parametrize("lat", LATTICES)
def test_labels_and_outcomes(lat):
    ref = reference(lat)
    with api.Context(*lat) as ctx:
        out = ctx.batch_bondc(ref["orders"], ref["trial"], ref["count"], solve=False)
    assert len(out) == len(ref["label"])
    seen = set()
    for o, li, tr, c in zip(out, ref["label"], ref["trial"], ref["count"]):
        for k in LABEL_KEYS:
            assert o[k] == li[k], (k, int(tr), int(c), o, li)
        assert o["fallback"] == (1 if li["nspan"] > 1 else 0), (int(tr), int(c), o, li)
        seen.add(min(li["nspan"], 2))
    # a batch that falls back everywhere must not pass: the share of items
    # several clusters span, on the single path's own count
    multi = sum(li["nspan"] > 1 for li in ref["label"])
    print("lattice %s: %d / %d items with nspan > 1" % (lat, multi, len(out)))
    assert multi <= 0.10 * len(out)
    assert {0, 1} <= seen  # nothing spans and one cluster spans both occur


@pytest.mark.parametrize("lat", LATTICES)
def test_literal_order_bitwise(lat):
    ref = reference(lat)
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        out = ctx.batch_bondc(ref["orders"], ref["trial"], ref["count"], tol=TOL, itmax=ITMAX)
    for o, c, tr, cnt in zip(out, ref["cond"], ref["trial"], ref["count"]):
        for k in COND_KEYS:
            assert o[k] == c[k], (k, int(tr), int(cnt), o, c)


def golden_trials(v):
    want, cur = [], None
    for line in G.text(v, "bondcond.txt").decode().splitlines():
        if "Trial #" in line:
            cur = dict(rows=[])
            want.append(cur)
        elif cur is not None and line.count(",") == 3:
            cur["rows"].append([float(x) for x in line.split(",")])
        elif "lattice-spanning cluster:" in line:
            cur["perccln"] = int(line.split(":")[1])
        elif "pc =" in line:
            cur["pc"] = float(line.split("=")[1])
    return want


@pytest.mark.parametrize("v", BOND_COND)
def test_ensemble_batch_literal_goldens(v):
    p = G.meta(v)["params"]
    with api.Ensemble(p["lattice"], p["m"], p["n"], p["pbc"], ndev=1, batch=64) as e:
        assert e.batch == 64
        e.set_dot_order(L.DOT_LITERAL)
        res, _ = e.bond_cond(p["seed"], p["numtrials"])
    want = golden_trials(v)
    assert len(res) == len(want)
    for tr, w in zip(res, want):
        assert len(tr["rows"]) == len(w["rows"])
        for r, wr in zip(tr["rows"], w["rows"]):
            assert "%12.9f" % r["pb"] == "%12.9f" % wr[0]
            assert abs(r["gbot"] - wr[1]) <= 2e-9 and abs(r["gtop"] - wr[2]) <= 2e-9, (r, wr)
        assert tr["pc"] == w["pc"] and tr["perccln"] == w["perccln"]


def rel(a, b):
    return abs(a - b) / abs(b)


_TIGHT = {}


def tight_literal(lat):
    """the literal results of reference(lat)'s items at tol 1e-13, for the
    truncation term of the accuracy bar.  They come from the batch kernel in
    the literal order, which test_literal_order_bitwise and test_size_edges
    pin to the single path bitwise; five items are checked against the single
    path here as well."""
    if lat in _TIGHT:
        return _TIGHT[lat]
    ref = reference(lat)
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        out = ctx.batch_bondc(ref["orders"], ref["trial"], ref["count"], tol=TIGHT, itmax=TIGHT_ITMAX)
        span = [i for i, li in enumerate(ref["label"]) if li["nspan"] == 1]
        for i in span[:: max(1, len(span) // 5)][:5]:
            _, c = single(ctx, ref["orders"][ref["trial"][i]], int(ref["count"][i]), tol=TIGHT,
                          itmax=TIGHT_ITMAX)
            assert all(out[i][k] == c[k] for k in COND_KEYS), (i, out[i], c)
    _TIGHT[lat] = out
    return out


def check_accuracy(got, ref, tight, what):
    """got (fast order, tol 1e-8) against the literal result ref at the same
    tol: rel. distance <= 2 trunc + max(1e-10, tol), trunc = the literal
    result's own relative move from that tol to 1e-13"""
    worst = 0.0
    for g in ("gtop", "gbot"):
        if ref[g] == 0.0:
            assert got[g] == 0.0, (what, g, got, ref)
            continue
        trunc = rel(ref[g], tight[g])
        d = rel(got[g], ref[g])
        worst = max(worst, d)
        assert d <= 2 * trunc + max(1e-10, TOL), (what, g, d, trunc, got, ref)
    return worst


def test_fast_order_deterministic_and_position_independent():
    lat = (0, 50, 50, 0)
    ref = reference(lat)
    nb = ref["nb"]
    grid = [int(c) for c in api.pb_grid(0, nb) if 0 < c <= nb]
    probe = (0, int(0.60 * nb))
    items = [probe] + [(i % 3, grid[(7 * i) % len(grid)]) for i in range(1, 299)] + [probe]
    it = np.array([x[0] for x in items], np.int32)
    ic = np.array([x[1] for x in items], np.int32)
    assert len(items) == 300
    with api.Context(*lat) as ctx:
        a = ctx.batch_bondc(ref["orders"], it, ic, tol=TOL, itmax=ITMAX)
        b = ctx.batch_bondc(ref["orders"], it, ic, tol=TOL, itmax=ITMAX)
    assert a == b  # two runs: bitwise
    assert a[0] == a[299] and a[0]["status"] == 0 and a[0]["iter"] > 0


def test_fast_order_accuracy():
    lat = (0, 50, 50, 0)
    ref = reference(lat)
    tight = tight_literal(lat)
    with api.Context(*lat) as ctx:
        out = ctx.batch_bondc(ref["orders"], ref["trial"], ref["count"], tol=TOL, itmax=ITMAX)
    worst = 0.0
    for i, (o, c) in enumerate(zip(out, ref["cond"])):
        assert o["status"] == c["status"]
        d = check_accuracy(o, c, tight[i], (int(ref["trial"][i]), int(ref["count"][i])))
        if c["status"] == 0:
            print("trial %d count %d: rel %.3e (iter %d, literal %d)"
                  % (ref["trial"][i], ref["count"][i], d, o["iter"], c["iter"]))
        worst = max(worst, d)
    print("worst relative distance to the literal result: %.3e" % worst)


@pytest.mark.parametrize("Va,g0,leak", R.NONUNIT, ids=["leak_dropped", "leak_kept"])
@pytest.mark.parametrize("lat", [(0, 10, 10, 0), (0, 50, 50, 0), (1, 12, 10, 1)])
def test_nonunit_values_literal_bitwise(lat, Va, g0, leak):
    """Va, g0 and leak that are no powers of two (no product exact), the
    leak below and above the 1e-10 threshold of the Fortran-rule currents
    (3e-9: the kernel's `>= 1e-10` keep branch runs): three trials at pb ~
    0.45, 0.6, 0.8 and 1.0 in the literal order, bitwise the single path with
    the same values and, on the 50 x 50 lattice, the oracle's linbcg and
    currents (or_bond_values / or_assemble / or_currents with g0, leak, Va)."""
    lattice, m, n, pbc = lat
    assert api.batch_supported(*lat)
    seeds = api.trial_seeds(58302, 3)
    b1, b2 = api.bond_list(*lat)
    nb = len(b1)
    orders = np.stack([api.shuffled_ids(nb, int(s)) for s in seeds])
    items = [(tr, int(pb * nb)) for tr in range(3) for pb in (0.45, 0.6, 0.8, 1.0)]
    it = np.array([x[0] for x in items], np.int32)
    ic = np.array([x[1] for x in items], np.int32)
    with api.Context(*lat) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        out = ctx.batch_bondc(orders, it, ic, Va=Va, g0=g0, leak=leak, tol=TOL, itmax=ITMAX)
        multi = spanning = 0
        for o, (tr, cnt) in zip(out, items):
            ctx.occupy(L.BOND, bond_order=orders[tr], nbonds_=cnt)
            li = ctx.label()
            c = ctx.conductance(L.RULE_BOND, L.CUR_FORTRAN, Va, g0, leak, 2, TOL, ITMAX)
            for k in LABEL_KEYS:
                assert o[k] == li[k], (k, tr, cnt, o, li)
            for k in COND_KEYS:
                assert o[k] == c[k], (k, tr, cnt, o, c)
            multi += li["nspan"] > 1
            if li["nspan"] == 0:
                assert o["status"] == 1 and o["gtop"] == 0.0 and o["gbot"] == 0.0
                continue
            spanning += 1
            assert o["status"] == 0 and o["gtop"] > 0.0 and o["iter"] <= ITMAX
            if (m, n) != (50, 50):
                continue
            ref = api.replay_labels(lattice, m, n, pbc, L.BOND, bond_order=orders[tr], nbond=cnt)
            gval = O.f64(nb)
            O.lib().or_bond_values(0, nb, b1, b2, ref["bond_label"], O.i32(1), ref["perccln"], g0, leak, gval)
            oc = O.conductance(lattice, m, n, pbc, b1, b2, gval, Va=Va, tol=TOL, itmax=ITMAX, cur_rule=0,
                               cur_thresh=1e-10)
            for k in ("gtop", "gbot", "iter", "err"):
                assert o[k] == oc[k], (k, tr, cnt, o[k], oc[k])
    print("lattice %s: %d / %d items span, %d with nspan > 1" % (lat, spanning, len(items), multi))
    assert spanning >= 6 and multi <= 0.10 * len(items)


@pytest.mark.parametrize("m,n", [(64, 130), (90, 93)])
def test_size_edges_literal_bitwise(m, n):
    """N = 8192 (the cap) and N = 8190 (no multiple of 64, a ragged last
    thread row): one trial at pb ~ 0.55 and pb = 1.0"""
    seed = int(api.trial_seeds(58302, 1)[0])
    with api.Context(0, m, n, 0) as ctx:
        nb = ctx.nb
        order = api.shuffled_ids(nb, seed)
        ctx.set_dot_order(L.DOT_LITERAL)
        counts = [int(0.55 * nb), nb]
        out = ctx.batch_bondc(order, [0, 0], counts, tol=TOL, itmax=ITMAX)
        for o, c in zip(out, counts):
            li, cr = single(ctx, order, c)
            assert li["nspan"] == 1
            for k in LABEL_KEYS:
                assert o[k] == li[k], (k, c, o, li)
            for k in COND_KEYS:
                assert o[k] == cr[k], (k, c, o, cr)


def test_unsupported_lattice_is_einval():
    with api.Context(0, 91, 93, 0) as ctx:
        order = api.shuffled_ids(ctx.nb, 1)
        with pytest.raises(L.PercError, match="PERC_EINVAL"):
            ctx.batch_bondc(order, [0], [ctx.nb // 2])
    with api.Context(0, 10, 10, 0) as ctx:
        order = api.shuffled_ids(ctx.nb, 1)
        for tr, cnt, itol in ((1, 5, 2), (-1, 5, 2), (0, ctx.nb + 2, 2), (0, -1, 2), (0, 5, 3), (0, 5, 4)):
            with pytest.raises(L.PercError, match="PERC_EINVAL"):
                ctx.batch_bondc(order, [tr], [cnt], itol=itol)


def column_bonds(m, n, col):
    b1, b2 = api.bond_list(0, m, n, 0)
    return [k + 1 for k in range(len(b1)) if b2[k] - b1[k] == m and (b1[k] - 1) % m == col]


def test_h2_spill_slot():
    """the shuffle's spill entry 0 inside the occupied prefix takes a
    position and is no bond"""
    m = n = 8
    nb = api.nbonds(0, m, n, 0)
    col = column_bonds(m, n, 3)
    ids = col[:2] + [0] + col[2:] + [k for k in range(1, nb + 1) if k not in col]
    order = np.array(ids, np.int32)
    assert len(order) == nb + 1 and order[2] == 0
    counts = [2, 3, 4, 7, 8, nb, nb + 1]
    with api.Context(0, m, n, 0) as ctx:
        ctx.set_dot_order(L.DOT_LITERAL)
        out = ctx.batch_bondc(order, [0] * len(counts), counts, tol=TOL, itmax=ITMAX)
        for o, c in zip(out, counts):
            li, cr = single(ctx, order, c)
            for k in LABEL_KEYS:
                assert o[k] == li[k], (k, c, o, li)
            for k in COND_KEYS:
                assert o[k] == cr[k], (k, c, o, cr)
    assert out[3]["nspan"] == 0 and out[4]["nspan"] == 1  # 6 / 7 bonds of the column


def test_forced_fallback():
    """two columns span at once: the reference's lowest-label rule through
    the single path"""
    m = n = 8
    nb = api.nbonds(0, m, n, 0)
    c0, c7 = column_bonds(m, n, 0), column_bonds(m, n, 7)
    assert len(c0) == len(c7) == 7
    rest = [k for k in range(1, nb + 1) if k not in c0 and k not in c7]
    order = np.array(c0 + c7 + rest + [0], np.int32)
    with api.Context(0, m, n, 0) as ctx:
        for solve in (False, True):
            o = ctx.batch_bondc(order, [0], [14], solve=solve, tol=TOL, itmax=ITMAX)[0]
            li, cr = single(ctx, order, 14, solve=solve)
            assert o["nspan"] == li["nspan"] == 2 and o["fallback"] == 1
            for k in LABEL_KEYS:
                assert o[k] == li[k], (k, o, li)
            if solve:
                for k in COND_KEYS:
                    assert o[k] == cr[k], (k, o, cr)
                assert o["gtop"] > 0.0
        # the other spanning column first: the lowest label follows the order
        order2 = np.array(c7 + c0 + rest + [0], np.int32)
        o2 = ctx.batch_bondc(order2, [0], [14], solve=False)[0]
        li2, _ = single(ctx, order2, 14, solve=False)
        assert o2["span_root"] == li2["span_root"] != o["span_root"]


def test_ensemble_batch_on_and_off():
    lat = (0, 50, 50, 0)
    with api.Ensemble(*lat, ndev=1, batch=256) as e:
        assert e.batch == 256
        on, son = e.bond_cond(58302, 3)
    with api.Ensemble(*lat, ndev=1) as e:
        assert e.batch == 0
        off, soff = e.bond_cond(58302, 3)
    ref, tight = reference(lat), tight_literal(lat)
    idx = {(int(t), int(c)): i for i, (t, c) in enumerate(zip(ref["trial"], ref["count"]))}
    assert len(on) == len(off) == 3
    for t, (a, b) in enumerate(zip(on, off)):
        assert [r["bf"] for r in a["rows"]] == [r["bf"] for r in b["rows"]] and a["rows"]
        assert a["bf_c"] == b["bf_c"] and a["pc"] == b["pc"] and a["perccln"] == b["perccln"]
        for r in a["rows"]:
            i = idx[t, r["bf"]]
            check_accuracy(r, ref["cond"][i], tight[i], (t, r["bf"]))
    assert np.array_equal(son[:, 0], soff[:, 0]) and np.array_equal(son[:, 3], soff[:, 3])


def test_ensemble_batch_ignored_on_large_lattice():
    lat = (0, 128, 128, 0)
    with api.Ensemble(*lat, ndev=1) as e:
        base, sbase = e.bond_cond(58302, 1)
        e.set_batch(256)
        assert e.batch == 0 and L.lib().perc_ensemble_batch(e.h) == 0
        got, sgot = e.bond_cond(58302, 1)
    assert got == base and np.array_equal(sgot, sbase)


def test_fortran_bond_cond_batch(tmp_path):
    v = "sq_bond_cond_3t"
    p = G.meta(v)["params"]
    exe = os.path.join(BIN, "bond_cond_sq")
    if not os.path.exists(exe):
        pytest.skip("Fortran drivers not built")
    (tmp_path / "bond_cond.nml").write_text(
        "&bond_cond_nml lattice=%d, m=%d, n=%d, pbc=%d, numtrials=%d, seed=%d, ndev=1, batch=64 /\n"
        % (p["lattice"], p["m"], p["n"], p["pbc"], p["numtrials"], p["seed"]))
    r = subprocess.run([exe], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = (tmp_path / "bondcond.txt").read_text().splitlines()
    want = G.text(v, "bondcond.txt").decode().splitlines()
    assert len(got) == len(want)
    rows = 0
    for a, b in zip(got, want):
        if b.count(",") == 3:
            fa, fb = [float(x) for x in a.split(",")], [float(x) for x in b.split(",")]
            assert a.split(",")[0] == b.split(",")[0]
            assert all(abs(x - y) <= 2e-9 for x, y in zip(fa[1:], fb[1:])), (a, b)
            rows += 1
        else:
            assert a == b
    assert rows > 0
