"""The march skips the bands the Krylov front has not reached.

A solve that starts from x0 = 0 has r0 nonzero on one lattice row (the
interior row next to the Va electrode); in iteration k, p is nonzero within
k - 1 rows of it and q, r within k rows, every other row an exact zero.  From
the second chunk of launches on (iteration 9) k_cg_march leaves out the bands
that miss the live rows the host hands it (perc_solve.hip, MarchFront): they
load nothing, store nothing and contribute +0.0 partials where they always
did.  Every nonzero of the solve must stay bitwise what it was.

Each test solves the same realisation on the same context with the front on
and off (PERC_MARCH_FRONT=0, read afresh by every solve) and requires
  * iter equal, the whole err history bitwise equal, Gtop and Gbot bitwise
    equal,
  * x on the two electrode-side rows equal as numbers (perc_x_row after the
    solve; -0.0 == +0.0: only the sign of a zero in a row the front never
    reached may differ),
  * last_solve(): front and front_iters > 0 where it is expected on, front
    false and front_iters 0 with the knob,
twice: on the metric's path (x carried on the electrode-side rows only) and
with every voltage kept (vint), whose values must be equal as numbers too.

Shapes.  128 x 128 is the smallest lattice at which test_literal_dot.py gets
the production strip-major march; its automatic bands hold 2 rows, 63 bands
per strip (asserted from march_info()).  The source row is the last interior
row, so with static bands of H rows band 0 stays dead through iteration
nrows - 2 - H (live rows of launch k: [nrows - 1 - (k + 1), nrows)), and
front_iters = min(iter, nrows - 2 - H) - 8 exactly.  128 x 300 with 43-row
bands (the metric's height) has bands that are partly live for many
iterations; 1024 x 530 gets the metric's slot-weighted bands whether a CU
holds 3 or 4 workgroups (128 cycles of 3 or 4 bands <= nrows: march_geometry).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import nr_systems as S
import oracle_lib as O
import rule_systems as R
from percolation_amd import _lib as PL
from percolation_amd import api

pytestmark = pytest.mark.gpu

MARCH_ONLY = PL.MARCH_DEFAULT & ~PL.SOLVE_RESIDENT
MARCH_ROWMAJOR = MARCH_ONLY & ~PL.MARCH_STRIPS
KNOB = "PERC_MARCH_FRONT"
FIRST_CHUNK = 8  # launches that walk every band (dev_solve_impl)

# (lattice, m, n, pbc, p, seed)
SQ128 = (0, 128, 128, 0, 0.6, 21)     # test_literal_dot.LATTICES[0]
TALL = (0, 128, 300, 0, 0.62, 43)     # more rows than columns (test_march_open.OPEN[0])
PBC = (0, 256, 67, 1, 0.60, 44)       # pbc columns: the run-time-mask instantiation
SLOTS = (0, 1024, 530, 0, 0.6, 5)     # slot-weighted bands
OTHER = (0, 128, 128, 0, 0.62, 77)    # a second realisation on SQ128's context


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture
def knob():
    """set(on): the front knob for the solves that follow; removed afterwards"""
    old = os.environ.get(KNOB)

    def set_(on):
        os.environ[KNOB] = "1" if on else "0"
    try:
        yield set_
    finally:
        if old is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = old


def occupy(ctx, case):
    lat, m, n, pbc, p, seed = case
    nb = api.nbonds(lat, m, n, pbc)
    ctx.occupy(PL.BOND, bond_order=api.shuffled_ids(nb, seed), nbonds_=int(p * nb))
    assert ctx.label()["nspan"] > 0, case


def electrode_rows(ctx):
    """x of the first and last interior rows as the solve left it"""
    nrows = ctx.n - 2
    buf = torch.empty(ctx.m, dtype=torch.float64, device="cuda:0")
    out = []
    for row in (0, nrows - 1):
        PL.check(PL.lib().perc_x_row(ctx.h, row, buf.data_ptr(), 0), "perc_x_row")
        out.append(buf.cpu().numpy().copy())
    return np.concatenate(out)


def solve(ctx, knob, on, **kw):
    knob(on)
    c = ctx.conductance(**kw)
    c["hist"] = ctx.err_history()
    c["ran"] = ctx.last_solve()
    c["rows"] = electrode_rows(ctx)
    return c


def assert_same(on, off, what, front=True):
    print(what, "iter", on["iter"], off["iter"], "gtop", on["gtop"], off["gtop"], "front_iters",
          on["ran"]["front_iters"])
    assert on["status"] == off["status"] == 0, what
    assert on["iter"] == off["iter"], (what, on["iter"], off["iter"])
    assert len(on["hist"]) == on["iter"] and np.array_equal(bits(on["hist"]), bits(off["hist"])), what
    assert bits(on["gtop"]) == bits(off["gtop"]) and bits(on["gbot"]) == bits(off["gbot"]), what
    assert bits(on["err"]) == bits(off["err"]), what
    assert np.array_equal(on["rows"], off["rows"]), what  # (as numbers)
    assert not np.isnan(on["rows"]).any(), what
    if "vint" in on:
        assert np.array_equal(on["vint"], off["vint"]) and not np.isnan(on["vint"]).any(), what
    assert not off["ran"]["front"] and off["ran"]["front_iters"] == 0, (what, off["ran"])
    assert on["ran"]["front"] == front, (what, on["ran"])
    assert (on["ran"]["front_iters"] > 0) == front, (what, on["ran"])
    drop = ("front", "front_iters")
    assert {k: v for k, v in on["ran"].items() if k not in drop} == \
        {k: v for k, v in off["ran"].items() if k not in drop}, what


def static_front_iters(ctx, it):
    """dead-band iterations of a solve of `it` iterations on static bands"""
    info = ctx.march_info()
    assert not info["slots"], info
    return max(0, min(it, ctx.n - 2 - 2 - info["band_rows"]) - FIRST_CHUNK)


def both_paths(ctx, knob, what, exact=True, **kw):
    """front on against front off, on the metric's path and with every
    voltage kept; returns the metric path's front-on solve"""
    first = None
    for vint in (False, True):
        off = solve(ctx, knob, False, vint=vint, **kw)
        on = solve(ctx, knob, True, vint=vint, **kw)
        assert_same(on, off, (what, "vint" if vint else "rows"))
        assert on["ran"]["kernel"] == "march" and on["ran"]["qfree"], on["ran"]
        if exact:
            assert on["ran"]["front_iters"] == static_front_iters(ctx, on["iter"]), (what, on["ran"])
        first = first or on
    return first


def at_least_three_bands(ctx):
    info = ctx.march_info()
    assert info["kernel"] == "wave" and 3 * info["band_rows"] <= ctx.n - 2, info
    return info


def test_spanning_realisation_to_tolerance(knob):
    """the front crosses the lattice long before convergence"""
    with api.Context(*SQ128[:4]) as ctx:
        ctx.set_march_mode(MARCH_ONLY)
        occupy(ctx, SQ128)
        c = both_paths(ctx, knob, "sq128", tol=1e-8, itmax=100000)
        info = at_least_three_bands(ctx)
        assert info["strips"] and info["nibble"] and c["ran"]["open"] and c["ran"]["tag"], (info, c["ran"])
        assert c["iter"] > 2 * (ctx.n - 2), c["iter"]


def test_itmax_20_stops_with_most_bands_dead(knob):
    """the solve stops after 21 iterations: bands 13 rows and more from the
    source never walked again after the first chunk; the x rows (the
    far one untouched since k_zero) and k_march_xpend's last update are
    still the parent's"""
    with api.Context(*SQ128[:4]) as ctx:
        ctx.set_march_mode(MARCH_ONLY)
        occupy(ctx, SQ128)
        c = both_paths(ctx, knob, "sq128-itmax20", tol=1e-8, itmax=20)
        at_least_three_bands(ctx)
        assert c["iter"] == 21 and c["ran"]["front_iters"] == 21 - FIRST_CHUNK, c["ran"]
        assert np.any(c["rows"] != 0.0)  # the source-side row moved


@pytest.mark.parametrize("case,rows", [(TALL, 0), (TALL, 43), (PBC, 0)], ids=["tall", "tall-rows43", "pbc"])
def test_rectangular_and_pbc(knob, case, rows):
    with api.Context(*case[:4]) as ctx:
        ctx.set_march_mode(MARCH_ONLY)
        ctx.set_march_rows(rows)
        occupy(ctx, case)
        for stop in ((1e-8, 100000), (1e-8, 60)):
            c = both_paths(ctx, knob, (case, rows, stop), tol=stop[0], itmax=stop[1])
        info = at_least_three_bands(ctx)
        assert c["ran"]["strips"] and c["ran"]["nibble"] and c["ran"]["open"] == (not case[3]), c["ran"]
        assert rows == 0 or info["band_rows"] == rows, info


def test_slot_weighted_bands(knob):
    """the metric's band split (PERC_MARCH_SLOTS), on the smallest lattice
    that gets it"""
    with api.Context(*SLOTS[:4]) as ctx:
        ctx.set_march_mode(MARCH_ONLY)
        occupy(ctx, SLOTS)
        for itmax in (100000, 150):
            c = both_paths(ctx, knob, ("slots", itmax), exact=False, tol=1e-8, itmax=itmax)
        info = ctx.march_info()
        assert info["slots"] and info["strips"] and c["ran"]["open"], (info, c["ran"])
        # 1-row bands, the far one dead until the live rows reach row 0
        assert c["iter"] == 151 and c["ran"]["front_iters"] == 151 - FIRST_CHUNK, c["ran"]


@pytest.mark.parametrize("rule", [PL.RULE_SITE, PL.RULE_MIXED], ids=["site", "mixed"])
@pytest.mark.parametrize("values", R.NONUNIT, ids=["leak-dropped", "leak-kept"])
def test_site_and_mixed_rules_nonunit_values(knob, rule, values):
    s = R.System(rule, *R.G_OPEN_SQ, *values)
    d = R.build(s)
    assert d["perccln"] > 0, R.name(s)
    with api.Context(*R.geometry(s)) as ctx:
        ctx.set_march_mode(MARCH_ONLY)
        ctx.occupy(**d["occ"])
        assert ctx.label()["nspan"] > 0
        kw = dict(rule=rule, cur_rule=R.natural_cur_rule(s), Va=s.Va, g0=s.g0, leak=s.leak)
        for itmax in (100000, 40):
            both_paths(ctx, knob, (R.name(s), itmax), tol=1e-8, itmax=itmax, **kw)
        at_least_three_bands(ctx)


def test_full_voltages(knob):
    """perc_set_full_voltages: x carried on every row by every B"""
    with api.Context(*SQ128[:4]) as ctx:
        ctx.set_march_mode(MARCH_ONLY)
        ctx.set_full_voltages(True)
        occupy(ctx, SQ128)
        for itmax in (100000, 50):
            off = solve(ctx, knob, False, tol=1e-8, itmax=itmax, vint=True)
            on = solve(ctx, knob, True, tol=1e-8, itmax=itmax, vint=True)
            assert_same(on, off, ("full", itmax))
            assert on["ran"]["front_iters"] == static_front_iters(ctx, on["iter"]), on["ran"]
        # (itmax 50: the rows the front never reached hold zeros)
        v = on["vint"].reshape(ctx.n - 2, ctx.m)
        assert np.all(v[:ctx.n - 2 - 60] == 0.0) and np.any(v[-1] != 0.0)


def test_row_major_march(knob):
    """MARCH_STRIPS off: the march of the vectors past the Infinity Cache
    shares the band test"""
    with api.Context(*SQ128[:4]) as ctx:
        ctx.set_march_mode(MARCH_ROWMAJOR)
        occupy(ctx, SQ128)
        for itmax in (100000, 30):
            c = both_paths(ctx, knob, ("rowmajor", itmax), tol=1e-8, itmax=itmax)
        at_least_three_bands(ctx)
        assert not c["ran"]["strips"] and c["ran"]["nibble"], c["ran"]


@pytest.mark.parametrize("order", [PL.DOT_LITERAL, PL.DOT_LITERAL_HOST], ids=["device-fold", "host-fold"])
def test_literal_dot_order_is_still_the_oracle_linbcg(knob, order):
    """the literal folds sum the term buffer over every row: the dead rows'
    terms are the zeros the first chunk's launches stored.  Front on: iter,
    the err history, Gtop and Gbot bitwise or_linbcg's, every voltage equal;
    and front on against front off at a stop inside the front's crossing"""
    lat, m, n, pbc, p, seed = SQ128
    b1, b2 = api.bond_list(lat, m, n, pbc)
    nb = len(b1)
    order_ids = api.shuffled_ids(nb, seed)
    tb = int(p * nb)
    ref = api.replay_labels(lat, m, n, pbc, PL.BOND, bond_order=order_ids, nbond=tb)
    assert ref["perccln"] > 0
    gval = O.f64(nb)
    O.lib().or_bond_values(0, nb, b1, b2, ref["bond_label"], O.i32(1), ref["perccln"], 1.0, 1e-12, gval)
    with api.Context(lat, m, n, pbc) as ctx:
        ctx.set_march_mode(MARCH_ONLY)
        ctx.set_dot_order(order)
        ctx.occupy(PL.BOND, bond_order=order_ids, nbonds_=tb)
        assert ctx.label()["nspan"] > 0
        for itmax in (100000, 40):
            oc = O.conductance(lat, m, n, pbc, b1, b2, gval, tol=1e-8, itmax=itmax)
            off = solve(ctx, knob, False, tol=1e-8, itmax=itmax, vint=True)
            on = solve(ctx, knob, True, tol=1e-8, itmax=itmax, vint=True)
            assert_same(on, off, ("literal", order, itmax))
            assert on["ran"]["literal"] and on["ran"]["lit_terms"] and on["ran"]["strips"], on["ran"]
            assert on["ran"]["host_fold"] == (order == PL.DOT_LITERAL_HOST), on["ran"]
            assert on["iter"] == oc["iter"], (itmax, on["iter"], oc["iter"])
            assert np.array_equal(bits(on["hist"]), bits(oc["errs"])), itmax
            assert on["gtop"] == oc["gtop"] and on["gbot"] == oc["gbot"], (itmax, on["gtop"], oc["gtop"])
            assert np.array_equal(on["vint"], oc["vint"]), itmax


def nr_last_solve():
    out = np.zeros(4, dtype=np.int32)
    PL.check(PL.lib().perc_nr_last_solve(out.ctypes.data), "perc_nr_last_solve")
    return int(out[1]), int(out[3])


@pytest.mark.parametrize("which", ["normal", "zero"])
def test_nonzero_start_through_the_nr_drop_in(which):
    """linbcg_ from x0 != 0 (and, on its general matrix, from x0 = 0): the
    front is off, and the solve is the oracle's literal linbcg bitwise"""
    n, maxrow, itol, tol, itmax = 1500, 4, 2, 1e-10, 5000
    rows, diag = S.sym_spd(n, maxrow, S.seed_of(n, maxrow), empty=S.edge_rows(n))
    sa, ija = S.to_nr(rows, diag)
    x0 = np.zeros(n) if which == "zero" else S.xvec(n, salt=1)
    assert (which == "zero") == (not np.any(x0))
    wx, wit, werr = O.nr_linbcg(sa, ija, S.bvec(n), x0, itol, tol, itmax)
    lib = PL.lib()
    b = np.array(S.bvec(n), dtype=np.float64, copy=True)
    x = np.array(x0, dtype=np.float64, copy=True)
    nn, it_, mx, it = C.c_int(n), C.c_int(itol), C.c_int(itmax), C.c_int(-1)
    tl, err = C.c_double(tol), C.c_double(-1.0)
    lib.perc_nr_set_dot_order(PL.DOT_LITERAL)
    lib.perc_nr_bind(sa.ctypes.data, ija.ctypes.data, len(sa))
    try:
        lib.linbcg_(C.byref(nn), b.ctypes.data, x.ctypes.data, C.byref(it_), C.byref(tl), C.byref(mx),
                    C.byref(it), C.byref(err))
    finally:
        lib.perc_nr_bind(None, None, 0)
    assert lib.perc_nr_status() == 0
    assert it.value == wit > FIRST_CHUNK and bits(err.value) == bits(werr), (it.value, wit)
    assert np.array_equal(bits(x), bits(wx))
    flags, front_iters = nr_last_solve()
    assert not flags & PL.RAN_FRONT and front_iters == 0, (flags, front_iters)


def test_two_solves_on_one_context(knob):
    """a realisation solved to convergence (every row of p, r, the edge pairs
    nonzero), then another stopped early and solved to the end: the second
    is its own front-off solve, nothing of the first leaks from the rows its
    dead bands leave alone"""
    with api.Context(*SQ128[:4]) as ctx:
        ctx.set_march_mode(MARCH_ONLY)
        occupy(ctx, SQ128)
        first = solve(ctx, knob, True, tol=1e-8, itmax=100000)
        assert first["ran"]["front_iters"] > 0 and first["iter"] > ctx.n
        occupy(ctx, OTHER)
        on = {}
        for itmax in (20, 100000):  # (front on right after the first realisation's solve)
            on[itmax] = solve(ctx, knob, True, tol=1e-8, itmax=itmax)
        for itmax in (20, 100000):
            assert_same(on[itmax], solve(ctx, knob, False, tol=1e-8, itmax=itmax), ("second", itmax))
        assert bits(on[100000]["gtop"]) != bits(first["gtop"])
        # and with the first realisation's long solve between each pair again
        occupy(ctx, SQ128)
        solve(ctx, knob, True, tol=1e-8, itmax=100000)
        occupy(ctx, OTHER)
        off = solve(ctx, knob, False, tol=1e-8, itmax=20)
        assert_same(on[20], off, "second after first, off")
