"""The configuration bench.py measures, held to the untimed host-order path.

The timed region of bench.py runs with kernel timing on
(perc_set_kernel_timing: every 64th iteration's launches go through klaunch's
event branch, the resident solve is bracketed by two events), with occupation
orders resident in device memory (perc_bondc_realisation(on_device=1),
perc_occupy_device), with one context reused across realisations and, under
--concurrent / --inflight, with several contexts in flight from one host
thread each.  Every other family is held bitwise to the oracle's linbcg or to
a path that is; this module extends that chain:

1. a timed solve is the untimed solve, bit for bit (iter, err, the whole err
   history, Gtop, Gbot, every voltage, perc_last_solve), at a tolerance stop
   and at an itmax stop whose last chunk has surplus no-op launches; the
   timed strip-major march in the literal dot order is the oracle's literal
   linbcg bitwise;
2. perc_kernel_stats obeys what perc.h and the chunk loop say (no measured
   constant): zero with timing off, reset, the resident solve's whole
   iterations, ceil(iter / 64) <= launches <= iter for the chunked loop,
   device times bounded by the solve's own wall time, nothing added by a
   realisation that does not span, accumulation over solves, and
   PERC_TIME_EVERY=1 (a fresh child process) counting exactly iter launches;
3. orders in device memory give the host path's occupancy, labels, replay
   and conductance exactly; perc_first_spanning / _mixed(on_device=1) give
   the host calls' counts; the device entry points refuse what the host ones
   refuse;
4. one context reused over six realisations (the third does not span) with
   timing on returns what a fresh untimed context returns for each alone;
5. K = 2 and K = 4 contexts in flight return what one serial context
   returned, realisation by realisation;
6. bench.py itself, once: the dumped results of its timed step are the API's
   on a fresh untimed context, and Gtop is the oracle's to the fast-order bar.

Shapes: the smallest at which each solver family runs (test_march_cmask.py,
test_march_open.py, test_slabs.py; oracle iterations at tol 1e-8 there).
Device buffers are torch int32 tensors on the context's device, synchronised
after creation and kept alive until the context has finished with them.
"""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import label_patterns as LP
import oracle_lib as O
from percolation_amd import _lib as PL
from percolation_amd import api

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(REPO, "tests")

MARCH_ONLY = PL.MARCH_DEFAULT & ~PL.SOLVE_RESIDENT   # as bench.py sets for K > 1
MARCH_ROWMAJOR = MARCH_ONLY & ~PL.MARCH_STRIPS
TIME_EVERY = 64  # perc.h: the CG launches of every 64th iteration of a chunk

# tag -> ((lattice, m, n, pbc), p, shuffle seed, march mode, format, slabs)
CASES = {
    "W": ((0, 50, 50, 0), 0.60, 41, PL.MARCH_DEFAULT, PL.FMT_AUTO, 1),      # one-workgroup solver
    "R": ((0, 128, 70, 0), 0.60, 41, PL.MARCH_DEFAULT, PL.FMT_AUTO, 1),     # resident solve
    "S1": ((0, 128, 70, 0), 0.60, 41, MARCH_ONLY, PL.FMT_AUTO, 1),          # strip-major march, 700 it.
    "S3": ((0, 384, 40, 0), 0.60, 42, MARCH_ONLY, PL.FMT_AUTO, 1),          # three strips, 563 it.
    "RM": ((0, 384, 40, 0), 0.60, 42, MARCH_ROWMAJOR, PL.FMT_AUTO, 1),      # row-major march
    "P": ((0, 256, 67, 1), 0.60, 44, MARCH_ONLY, PL.FMT_AUTO, 1),           # strip-major under pbc
    "T": ((1, 128, 80, 0), 0.42, 45, MARCH_ONLY, PL.FMT_AUTO, 1),           # triangular (u16 codes)
    "C": ((0, 128, 70, 0), 0.60, 41, PL.MARCH_DEFAULT, PL.FMT_CSR, 1),      # unfused loop, CSR
    "SP": ((0, 128, 70, 0), 0.60, 41, PL.MARCH_DEFAULT, PL.FMT_STENCIL_SPLIT, 1),  # unfused, stencil
    "SL": ((0, 128, 128, 0), 0.60, 21, PL.MARCH_DEFAULT, PL.FMT_AUTO, 2),   # slab solve
}
TAGS = list(CASES)
LAUNCHED = ("S1", "S3", "RM", "P", "T", "C", "SP")  # the chunked loop: sampled launches
UNFUSED = ("C", "SP")                               # ... with k_cg_p launched and timed
UNSAMPLED = ("W", "SL")                             # one launch / slab loop: no timing code
# (tol, itmax): a tolerance stop; an itmax stop at iter 101 (linbcg counts to
# itmax + 1, bondc.f:780) -- chunks of 8, 16, 32, 64 launches, so the last
# chunk has 19 surplus no-op launches
STOPS = ((1e-8, 10 ** 6), (1e-300, 100))

_ORDER = {}
_PAIR = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def dev(a):
    """an int32 array as a torch tensor on the contexts' device (cuda:0)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def order_of(tag):
    """(bond order, count) of the case; it spans (asserted on the CPU)"""
    if tag not in _ORDER:
        (lat, m, n, pbc), p, seed = CASES[tag][:3]
        nb = api.nbonds(lat, m, n, pbc)
        order = api.shuffled_ids(nb, seed)
        tb = int(p * nb)
        assert api.replay_labels(lat, m, n, pbc, PL.BOND, bond_order=order, nbond=tb)["perccln"] > 0, tag
        _ORDER[tag] = (order, tb)
    return _ORDER[tag]


def make_ctx(tag):
    geom, _, _, mode, fmt, slabs = CASES[tag]
    ctx = api.Context(*geom)
    ctx.set_matrix_format(fmt)
    ctx.set_march_mode(mode)
    if slabs > 1:
        ctx.set_slabs(slabs)
    return ctx


def check_family(tag, ctx):
    """the solver family the case is there for ran the last solve"""
    ran, info = ctx.last_solve(), ctx.march_info()
    what = (tag, ran, info)
    if tag == "W":
        assert ran["kernel"] == "small" and info["kernel"] == "small", what
    elif tag == "R":
        assert ran["kernel"] == "resident" and info["kernel"] == "resident", what
    elif tag in ("S1", "S3"):
        assert ran["kernel"] == "march" and ran["qfree"] and ran["strips"] and ran["nibble"] and ran["open"], what
        assert info["kernel"] == "wave" and info["strips"], what
    elif tag == "RM":
        assert ran["kernel"] == "march" and ran["qfree"] and not ran["strips"] and not ran["open"], what
    elif tag == "P":
        assert ran["kernel"] == "march" and ran["qfree"] and ran["strips"] and ran["nibble"] and not ran["open"], what
    elif tag == "T":
        assert ran["kernel"] == "march" and ran["qfree"] and ran["strips"] and not ran["nibble"], what
    elif tag == "C":
        assert ran["kernel"] == "other" and ctx.matrix_format() == PL.FMT_CSR, what
    elif tag == "SP":
        assert ran["kernel"] == "other" and ctx.matrix_format() == PL.FMT_STENCIL_SPLIT, what
    else:
        assert tag == "SL" and ran["kernel"] == "slabs", what


def solve(ctx, stop, **kw):
    tol, itmax = stop
    c = ctx.conductance(tol=tol, itmax=itmax, vint=True, **kw)
    c["hist"] = ctx.err_history()
    c["ran"] = ctx.last_solve()
    return c


def assert_same_solve(a, b, what):
    assert a["iter"] == b["iter"] and a["status"] == b["status"] == 0, (what, a["iter"], b["iter"])
    for k in ("err", "gtop", "gbot"):
        assert same_bits(a[k], b[k]), (what, k, a[k], b[k])
    assert len(a["hist"]) == a["iter"] and same_bits(a["hist"], b["hist"]), what
    assert same_bits(a["vint"], b["vint"]), what
    assert a["ran"] == b["ran"], (what, a["ran"], b["ran"])


def counts(st):
    return (st["spmv_n"], st["resid_n"], st["xp_n"])


def all_zero(st):
    return counts(st) == (0, 0, 0) and st["spmv_ms"] == 0.0 and st["resid_ms"] == 0.0 and st["xp_ms"] == 0.0


def check_stats(tag, st, iters, t_solve_ms):
    """perc_kernel_stats after timed solves of `iters` iterations (a list:
    one entry per solve) whose t_solve_ms sum to t_solve_ms"""
    total = sum(iters)
    what = (tag, st, iters, t_solve_ms)
    if tag in UNSAMPLED:
        assert all_zero(st), what
    elif tag == "R":  # whole iterations between the two events around the launch
        assert st["spmv_n"] == total and st["resid_n"] == 0 and st["xp_n"] == 0, what
        assert 0.0 < st["spmv_ms"] <= t_solve_ms, what
        assert st["resid_ms"] == 0.0 and st["xp_ms"] == 0.0, what
    else:
        assert tag in LAUNCHED
        assert st["spmv_n"] == st["resid_n"] == st["xp_n"], what
        assert sum(-(-i // TIME_EVERY) for i in iters) <= st["spmv_n"] <= total, what
        assert np.isfinite(st["spmv_ms"]) and st["spmv_ms"] > 0.0, what
        assert np.isfinite(st["resid_ms"]) and st["resid_ms"] > 0.0, what
        if tag in UNFUSED:
            assert np.isfinite(st["xp_ms"]) and st["xp_ms"] > 0.0, what
        else:
            assert st["xp_ms"] == 0.0, what
        # sequential launches on one stream inside the solve's own events
        assert st["spmv_ms"] + st["resid_ms"] + st["xp_ms"] <= t_solve_ms, what


def timed_pair(tag):
    """per stop: the untimed and the timed solve of the case on one context,
    with the statistics read after each (computed once per case)"""
    if tag in _PAIR:
        return _PAIR[tag]
    order, tb = order_of(tag)
    out = {}
    with make_ctx(tag) as ctx:
        ctx.occupy(PL.BOND, bond_order=order, nbonds_=tb)
        assert ctx.label()["nspan"] > 0, tag
        first = ctx.kernel_stats(reset=False)
        for stop in STOPS:
            ctx.set_kernel_timing(False)
            off = solve(ctx, stop)
            check_family(tag, ctx)
            st_off = ctx.kernel_stats(reset=False)
            ctx.set_kernel_timing(True)
            on = solve(ctx, stop)
            check_family(tag, ctx)
            st_on = ctx.kernel_stats(reset=True)
            st_reset = ctx.kernel_stats(reset=False)
            out[stop] = dict(off=off, on=on, st_off=st_off, st_on=st_on, st_reset=st_reset)
        out["first"] = first
    _PAIR[tag] = out
    return out


# ------------------------------------------------ 1. timed == untimed
@pytest.mark.parametrize("tag", TAGS)
def test_timed_solve_is_the_untimed_solve_bitwise(tag):
    pair = timed_pair(tag)
    for stop in STOPS:
        off, on = pair[stop]["off"], pair[stop]["on"]
        print(tag, stop, "iter", off["iter"], on["iter"], "gtop", off["gtop"], on["gtop"])
        assert_same_solve(off, on, (tag, stop))
    assert pair[STOPS[0]]["off"]["iter"] > 50, tag
    assert pair[STOPS[1]]["off"]["iter"] == STOPS[1][1] + 1, (tag, pair[STOPS[1]]["off"]["iter"])


_LIT_ORACLE = {}


def s1_oracle(tol):
    if tol not in _LIT_ORACLE:
        (lat, m, n, pbc), _, _ = CASES["S1"][:3]
        order, tb = order_of("S1")
        b1, b2 = api.bond_list(lat, m, n, pbc)
        ref = api.replay_labels(lat, m, n, pbc, PL.BOND, bond_order=order, nbond=tb)
        gval = O.f64(len(b1))
        O.lib().or_bond_values(0, len(b1), b1, b2, ref["bond_label"], O.i32(1), ref["perccln"], 1.0, 1e-12, gval)
        _LIT_ORACLE[tol] = O.conductance(lat, m, n, pbc, b1, b2, gval, tol=tol, itmax=100000)
    return _LIT_ORACLE[tol]


def test_timed_literal_march_is_the_oracle_linbcg_bitwise():
    """the timed launch path on the oracle directly: S1 under PERC_DOT_LITERAL
    with kernel timing on (test_march_open.py's protocol)"""
    order, tb = order_of("S1")
    with make_ctx("S1") as ctx:
        ctx.set_dot_order(PL.DOT_LITERAL)
        ctx.set_kernel_timing(True)
        ctx.occupy(PL.BOND, bond_order=order, nbonds_=tb)
        assert ctx.label()["nspan"] > 0
        for tol in (1e-8, 1e-13):
            oc = s1_oracle(tol)
            c = ctx.conductance(tol=tol, itmax=100000, vint=True)
            hist = ctx.err_history()
            ran = ctx.last_solve()
            st = ctx.kernel_stats(reset=True)
            assert ran["kernel"] == "march" and ran["literal"] and ran["lit_terms"], ran
            assert ran["qfree"] and ran["strips"] and ran["nibble"] and ran["open"], ran
            print("literal", tol, c["iter"], oc["iter"], c["gtop"], oc["gtop"], st)
            assert c["iter"] == oc["iter"] == ran["iter"], (tol, c["iter"], oc["iter"])
            assert same_bits(hist, oc["errs"]), tol
            assert same_bits(c["gtop"], oc["gtop"]) and same_bits(c["gbot"], oc["gbot"]), (tol, c["gtop"], oc["gtop"])
            assert same_bits(c["vint"], oc["vint"]), tol
            check_stats("S1", st, [c["iter"]], c["t_solve_ms"])


# ------------------------------------------------ 2. perc_kernel_stats
@pytest.mark.parametrize("tag", TAGS)
def test_kernel_stats_obey_the_loop(tag):
    """W and SL: perc.h's sampled launches are the chunked loop's, and the
    one-workgroup solve and the slab solve return before it (dev_solve_impl):
    every field stays 0."""
    pair = timed_pair(tag)
    assert all_zero(pair["first"]), (tag, pair["first"])
    for stop in STOPS:
        d = pair[stop]
        print(tag, stop, d["on"]["iter"], d["on"]["t_solve_ms"], d["st_on"])
        assert all_zero(d["st_off"]), (tag, stop, d["st_off"])      # timing off: nothing recorded
        assert all_zero(d["st_reset"]), (tag, stop, d["st_reset"])  # reset zeroed the accumulators
        check_stats(tag, d["st_on"], [d["on"]["iter"]], d["on"]["t_solve_ms"])


@pytest.mark.parametrize("tag", ["R", "S1", "C"])
def test_kernel_stats_accumulate_over_solves(tag):
    """two timed solves without a reset: the counts are the sum of the two
    solves' separate counts; a realisation that does not span adds nothing"""
    pair = timed_pair(tag)
    sep = [pair[stop]["st_on"] for stop in STOPS]
    order, tb = order_of(tag)
    geom = CASES[tag][0]
    tb40 = int(0.40 * api.nbonds(*geom))
    assert api.replay_labels(*geom, PL.BOND, bond_order=order, nbond=tb40)["perccln"] == 0
    with make_ctx(tag) as ctx:
        ctx.set_kernel_timing(True)
        ctx.occupy(PL.BOND, bond_order=order, nbonds_=tb)
        assert ctx.label()["nspan"] > 0
        res = [solve(ctx, stop) for stop in STOPS]
        st = ctx.kernel_stats(reset=False)
        assert counts(st) == tuple(a + b for a, b in zip(counts(sep[0]), counts(sep[1]))), (st, sep)
        check_stats(tag, st, [r["iter"] for r in res], sum(r["t_solve_ms"] for r in res))
        # p = 0.40: nothing spans, no solve, the accumulators stay
        ctx.occupy(PL.BOND, bond_order=order, nbonds_=tb40)
        assert ctx.label()["nspan"] == 0
        c = ctx.conductance(tol=1e-8, itmax=10 ** 6)
        assert c["status"] == 1 and c["iter"] == 0 and c["gtop"] == 0.0 and c["gbot"] == 0.0, c
        again = ctx.kernel_stats(reset=True)
        assert counts(again) == counts(st), (again, st)
        assert (again["spmv_ms"], again["resid_ms"], again["xp_ms"]) == (st["spmv_ms"], st["resid_ms"], st["xp_ms"])
        assert all_zero(ctx.kernel_stats(reset=False))
        ctx.conductance(tol=1e-8, itmax=10 ** 6)
        assert all_zero(ctx.kernel_stats(reset=False))


def child_time_every():
    """run in a fresh process with PERC_TIME_EVERY=1: S1 and the unfused C at
    both stops with kernel timing on; one JSON line"""
    out = {}
    for tag in ("S1", "C"):
        order, tb = order_of(tag)
        with make_ctx(tag) as ctx:
            ctx.set_kernel_timing(True)
            ctx.occupy(PL.BOND, bond_order=order, nbonds_=tb)
            assert ctx.label()["nspan"] > 0
            for k, stop in enumerate(STOPS):
                c = solve(ctx, stop)
                check_family(tag, ctx)
                st = ctx.kernel_stats(reset=True)
                out["%s/%d" % (tag, k)] = dict(
                    iter=c["iter"], gtop=bits(c["gtop"]).tolist(), gbot=bits(c["gbot"]).tolist(),
                    err=bits(c["err"]).tolist(), hist=bits(c["hist"]).tolist(), vint=bits(c["vint"]).tolist(),
                    t_solve_ms=c["t_solve_ms"], stats={k_: float(v) for k_, v in st.items()})
    print("TIME_EVERY " + json.dumps(out), flush=True)


def test_time_every_1_counts_every_iteration_and_no_surplus_launch():
    """PERC_TIME_EVERY is read once per process: a fresh child runs S1 and C
    with every iteration's launches timed.  The launches counted are exactly
    iter of each kind -- the surplus no-op launches of the last chunk are left
    out -- and the numbers are the parent's untimed ones."""
    env = dict(os.environ, PERC_TIME_EVERY="1")
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_bench_path as T; T.child_time_every()"
            % (REPO, TESTS))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, cwd=REPO,
                       env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("TIME_EVERY ")]
    assert len(lines) == 1, r.stdout[-2000:]
    got = json.loads(lines[0][len("TIME_EVERY "):])
    for tag in ("S1", "C"):
        pair = timed_pair(tag)
        for k, stop in enumerate(STOPS):
            g, off = got["%s/%d" % (tag, k)], pair[stop]["off"]
            st = g["stats"]
            print(tag, stop, g["iter"], st)
            assert g["iter"] == off["iter"], (tag, stop, g["iter"], off["iter"])
            assert st["spmv_n"] == st["resid_n"] == st["xp_n"] == g["iter"], (tag, stop, st)
            for key in ("gtop", "gbot", "err", "hist", "vint"):
                assert np.array_equal(np.array(g[key], dtype=np.uint64), bits(off[key])), (tag, stop, key)
            assert st["spmv_ms"] > 0.0 and st["resid_ms"] > 0.0, st
            assert (st["xp_ms"] > 0.0) == (tag in UNFUSED), st
            assert st["spmv_ms"] + st["resid_ms"] + st["xp_ms"] <= g["t_solve_ms"], (st, g["t_solve_ms"])


# ------------------------------------------------ 3. orders in device memory
KINDS = ("bond", "site", "mixed")
KIND_ID = {"bond": PL.BOND, "site": PL.SITE, "mixed": PL.SITEBOND}
RULES = {"bond": (PL.RULE_BOND, PL.CUR_FORTRAN), "site": (PL.RULE_SITE, PL.CUR_MATLAB),
         "mixed": (PL.RULE_MIXED, PL.CUR_MATLAB)}   # as bench.py pairs them
PS_SITE, P_MIXED = 0.66, (0.90, 0.80)
DEV_TAGS = ("W", "S1", "T")
# shuffle seeds whose spill slot (the 0 of the N + 1 entries, hazard H2) lands
# inside the first N entries: list length N -> seed (asserted where used)
SPILL_SEED = {4900: 1872, 2500: 1033, 17722: 52, 8960: 124, 30305: 9, 10240: 172}


def kind_counts(tag, kind):
    """(site count, bond count) of the case's spanning occupancy of a kind"""
    geom, p = CASES[tag][:2]
    t, nb = geom[1] * geom[2], api.nbonds(*geom)
    if kind == "bond":
        return 0, int(p * nb)
    if kind == "site":
        return int(PS_SITE * t), 0
    return int(P_MIXED[0] * t), int(P_MIXED[1] * nb)


def kind_orders(tag, kind):
    """(site order, bond order) of the case (lists of N + 1 entries); the
    occupancy of kind_counts spans (asserted on the CPU)"""
    geom, _, seed = CASES[tag][:3]
    t, nb = geom[1] * geom[2], api.nbonds(*geom)
    so = api.shuffled_ids(t, seed + 100) if kind != "bond" else None
    bo = api.shuffled_ids(nb, seed) if kind != "site" else None
    ns, nbo = kind_counts(tag, kind)
    r = api.replay_labels(*geom, KIND_ID[kind], site_order=so, nsites=ns, bond_order=bo, nbond=nbo)
    assert r["perccln"] > 0, (tag, kind)
    return so, bo


def spill_order(N):
    """(order, position of the spill slot) of a shuffle whose 0 lies inside
    the first N entries"""
    o = api.shuffled_ids(N, SPILL_SEED[N])
    pos = int(np.nonzero(o == 0)[0][0])
    assert pos < N, (N, pos)
    return o, pos


def occupy_both(hctx, dctx, kind, so, ns, bo, nbo, keep):
    """the same occupation through perc_occupy on hctx and perc_occupy_device
    on dctx (device tensors appended to keep)"""
    k = KIND_ID[kind]
    hctx.occupy(k, site_order=so, nsites=ns, bond_order=bo, nbonds_=nbo)
    ds = dev(so) if so is not None else None
    db = dev(bo) if bo is not None else None
    keep += [ds, db]
    dctx.occupy_device(k, ds.data_ptr() if ds is not None else None, ns,
                       db.data_ptr() if db is not None else None, nbo)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tag", DEV_TAGS)
def test_occupy_device_is_the_host_occupancy(tag, kind):
    """perc_occupy_device against perc_occupy on a context of its own (its
    upload buffer never holds the order): counts 0, 1, the case's, one past
    the spill slot of an order that has it inside, and the whole order"""
    geom = CASES[tag][0]
    t, nb = geom[1] * geom[2], api.nbonds(*geom)
    so, bo = kind_orders(tag, kind)
    ns, nbo = kind_counts(tag, kind)
    trials = [(so, 0, bo, 0), (so, min(ns, 1), bo, min(nbo, 1)), (so, ns, bo, nbo)]
    sso, spos = spill_order(t) if kind != "bond" else (None, -1)
    sbo, bpos = spill_order(nb) if kind != "site" else (None, -1)
    trials += [(sso, spos + 1, sbo, bpos + 1), (sso, t if kind != "bond" else 0, sbo, nb if kind != "site" else 0)]
    keep = []
    with make_ctx(tag) as hctx, make_ctx(tag) as dctx:
        for s_, ns_, b_, nb_ in trials:
            occupy_both(hctx, dctx, kind, s_, ns_, b_, nb_, keep)
            hs, hb = hctx.occupancy()
            ds, db = dctx.occupancy()
            assert np.array_equal(hs, ds) and np.array_equal(hb, db), (tag, kind, ns_, nb_)
            # the spill slot is no element: the prefix past it holds one id less
            want_s = np.count_nonzero(s_[:ns_]) if kind != "bond" else 0
            want_b = np.count_nonzero(b_[:nb_]) if kind != "site" else 0
            assert (int(ds.sum()), int(db.sum())) == (want_s, want_b), (tag, kind, ns_, nb_)
    del keep


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tag", DEV_TAGS)
def test_device_order_solve_is_the_host_order_solve_bitwise(tag, kind):
    so, bo = kind_orders(tag, kind)
    ns, nbo = kind_counts(tag, kind)
    rule, cur = RULES[kind]
    keep = []
    with make_ctx(tag) as hctx, make_ctx(tag) as dctx:
        occupy_both(hctx, dctx, kind, so, ns, bo, nbo, keep)
        hl, dl = hctx.label(canon=True), dctx.label(canon=True)
        assert hl["nspan"] > 0, (tag, kind)
        assert np.array_equal(hl.pop("canon"), dl.pop("canon")), (tag, kind)
        assert hl == dl, (tag, kind, hl, dl)
        stop = (1e-8, 10 ** 5)
        hc = solve(hctx, stop, rule=rule, cur_rule=cur)
        dc = solve(dctx, stop, rule=rule, cur_rule=cur)
        print(tag, kind, hc["iter"], hc["gtop"], dc["gtop"], hc["ran"])
        assert_same_solve(hc, dc, (tag, kind))
        if kind == "bond":
            check_family(tag, dctx)
    del keep


@pytest.mark.parametrize("kind", ["bond", "mixed"])
def test_device_order_replay_arm(kind):
    """several spanning clusters (vertical stripes): the lowest-label rule
    needs the host replay, which fetches a device-resident order back"""
    geom = (0, 128, 70, 0)
    bids = LP.ordered(LP.bond_ids("vstripes", *geom), "perm", 7)
    sids = LP.ordered(LP.site_ids("vstripes", geom[1], geom[2]), "perm", 8) if kind == "mixed" else None
    rule, cur = RULES[kind]
    keep = []
    with api.Context(*geom) as hctx, api.Context(*geom) as dctx:
        occupy_both(hctx, dctx, kind, sids, len(sids) if sids is not None else 0, bids, len(bids), keep)
        hl, dl = hctx.label(), dctx.label()
        assert hl["nspan"] > 1 and hl["replayed"] == 1 and hl["perccln"] > 0, hl
        assert dl["replayed"] == 1, dl
        for k in ("nspan", "span_root", "perccln"):
            assert hl[k] == dl[k], (k, hl, dl)
        assert hl == dl, (hl, dl)
        hn, dn = hctx.label_numbers(KIND_ID[kind]), dctx.label_numbers(KIND_ID[kind])
        for k in ("bond_label", "site_label", "csize"):
            assert (hn[k] is None and dn[k] is None) or np.array_equal(hn[k], dn[k]), (kind, k)
        assert hn["perccln"] == dn["perccln"] == hl["perccln"], (hn["perccln"], dn["perccln"])
        assert (hn["cln"], hn["maxcn"], hn["maxcs"]) == (dn["cln"], dn["maxcn"], dn["maxcs"])
        stop = (1e-8, 10 ** 5)
        assert_same_solve(solve(hctx, stop, rule=rule, cur_rule=cur), solve(dctx, stop, rule=rule, cur_rule=cur),
                          kind)
    del keep


LABEL_KEYS = [k for k, _ in PL.LabelInfo._fields_]
COND_KEYS = ("gtop", "gbot", "err", "iter", "status")


def assert_same_realisation(a, b, what):
    for k in LABEL_KEYS:
        assert a[k] == b[k], (what, k, a[k], b[k])
    assert a["iter"] == b["iter"] and a["status"] == b["status"], (what, a["iter"], b["iter"])
    for k in ("gtop", "gbot", "err"):
        assert same_bits(a[k], b[k]), (what, k, a[k], b[k])


@pytest.mark.parametrize("tag", DEV_TAGS)
def test_bondc_realisation_device_order(tag):
    order, tb = order_of(tag)
    d_order = dev(order)
    with make_ctx(tag) as dctx, make_ctx(tag) as hctx, make_ctx(tag) as sctx:
        rd = dctx.bondc_realisation(None, tb, device_ptr=d_order.data_ptr())
        check_family(tag, dctx)
        rh = hctx.bondc_realisation(order, tb)
        sctx.occupy(PL.BOND, bond_order=order, nbonds_=tb)
        rs = sctx.label()
        rs.update(sctx.conductance(PL.RULE_BOND, PL.CUR_FORTRAN, Va=1.0, g0=1.0, leak=1e-12, itol=2, tol=1e-8,
                                   itmax=2500))
        assert rd["nspan"] > 0 and rd["status"] == 0 and rd["iter"] > 50, rd
        assert_same_realisation(rd, rh, (tag, "host order"))
        assert_same_realisation(rd, rs, (tag, "occupy + label + conductance"))
        for r in (rd, rh):
            assert 0.0 <= r["t_upload_ms"] and 0.0 <= r["t_label_ms"], r
            assert r["t_upload_ms"] + r["t_label_ms"] <= r["t_total_ms"], r
    del d_order


SCAN_GEOMS = [(0, 33, 31, 0), (1, 64, 40, 1)]


@pytest.mark.parametrize("kind", ["bond", "site"])
@pytest.mark.parametrize("geom", SCAN_GEOMS, ids=["sq33x31", "tri64x40pbc"])
def test_first_spanning_on_device(geom, kind):
    k = KIND_ID[kind]
    N = api.nbonds(*geom) if kind == "bond" else geom[1] * geom[2]
    order = api.shuffled_ids(N, 7 if kind == "bond" else 8)[:N]
    d_order = dev(order)
    with api.Context(*geom) as hctx, api.Context(*geom) as dctx:
        hf = api.first_spanning(hctx, order, k, N)
        df = api.first_spanning(dctx, d_order.data_ptr(), k, N, on_device=True)
        assert 0 < hf == df, (hf, df)
        assert hctx.cluster_sizes() == dctx.cluster_sizes()
        hl, dl = hctx.label(canon=True), dctx.label(canon=True)
        assert np.array_equal(hl.pop("canon"), dl.pop("canon"))
        assert hl == dl and hl["nspan"] > 0, (hl, dl)
        hn, dn = hctx.label_numbers(k), dctx.label_numbers(k)
        for key in ("bond_label", "site_label", "csize"):
            assert (hn[key] is None and dn[key] is None) or np.array_equal(hn[key], dn[key]), key
        assert hn["perccln"] == dn["perccln"] > 0
    del d_order


@pytest.mark.parametrize("scan", ["bond", "site"])
@pytest.mark.parametrize("geom", SCAN_GEOMS, ids=["sq33x31", "tri64x40pbc"])
def test_first_spanning_mixed_on_device(geom, scan):
    t, nb = geom[1] * geom[2], api.nbonds(*geom)
    so, bo = api.shuffled_ids(t, 9)[:t], api.shuffled_ids(nb, 10)[:nb]
    ns, nbo = (int(0.90 * t), nb) if scan == "bond" else (t, int(0.80 * nb))
    assert api.replay_labels(*geom, PL.SITEBOND, site_order=so, nsites=ns, bond_order=bo, nbond=nbo)["perccln"] > 0
    ds, db = dev(so), dev(bo)
    with api.Context(*geom) as hctx, api.Context(*geom) as dctx:
        hf = api.first_spanning_mixed(hctx, KIND_ID[scan], so, ns, bo, nbo)
        df = api.first_spanning_mixed(dctx, KIND_ID[scan], ds.data_ptr(), ns, db.data_ptr(), nbo, on_device=True)
        assert 0 < hf == df, (hf, df)
        for ctx in (hctx, dctx):  # the context is left unoccupied
            with pytest.raises(PL.PercError, match="PERC_ESTATE"):
                ctx.label()
    del ds, db


def test_device_entry_points_refuse_what_the_host_ones_refuse():
    import ctypes as C
    lib = PL.lib()
    geom = (0, 33, 31, 0)
    t, nb = geom[1] * geom[2], api.nbonds(*geom)
    so, bo = api.shuffled_ids(t, 9), api.shuffled_ids(nb, 10)
    ds, db = dev(so), dev(bo)
    first, real = C.c_int(), PL.Realisation()
    with api.Context(*geom) as ctx:
        for on_dev, sp, bp in ((0, PL.ptr(so), PL.ptr(bo)), (1, C.c_void_p(ds.data_ptr()), C.c_void_p(db.data_ptr()))):
            occ = lib.perc_occupy_device if on_dev else lib.perc_occupy
            bad = [
                occ(ctx.h, PL.BOND, 0, None, -1, bp), occ(ctx.h, PL.SITE, -1, sp, 0, None),
                occ(ctx.h, PL.BOND, 0, None, nb + 1, bp), occ(ctx.h, PL.SITE, t + 1, sp, 0, None),
                occ(ctx.h, PL.BOND, 0, None, 5, None), occ(ctx.h, PL.SITEBOND, 5, None, 5, bp),
                occ(None, PL.BOND, 0, None, 5, bp),
                lib.perc_bondc_realisation(ctx.h, -1, bp, on_dev, 1.0, 1.0, 1e-8, 100, C.byref(real)),
                lib.perc_bondc_realisation(ctx.h, nb + 1, bp, on_dev, 1.0, 1.0, 1e-8, 100, C.byref(real)),
                lib.perc_bondc_realisation(ctx.h, 5, None, on_dev, 1.0, 1.0, 1e-8, 100, C.byref(real)),
                lib.perc_bondc_realisation(None, 5, bp, on_dev, 1.0, 1.0, 1e-8, 100, C.byref(real)),
                lib.perc_first_spanning(ctx.h, PL.BOND, bp, -1, on_dev, C.byref(first)),
                lib.perc_first_spanning(ctx.h, PL.BOND, bp, nb + 1, on_dev, C.byref(first)),
                lib.perc_first_spanning(ctx.h, PL.SITE, sp, t + 1, on_dev, C.byref(first)),
                lib.perc_first_spanning(ctx.h, PL.BOND, None, 5, on_dev, C.byref(first)),
                lib.perc_first_spanning(None, PL.BOND, bp, 5, on_dev, C.byref(first)),
                lib.perc_first_spanning_mixed(ctx.h, PL.BOND, sp, -1, bp, 5, on_dev, C.byref(first)),
                lib.perc_first_spanning_mixed(ctx.h, PL.BOND, sp, 5, bp, nb + 1, on_dev, C.byref(first)),
                lib.perc_first_spanning_mixed(ctx.h, PL.SITE, sp, t + 1, bp, 5, on_dev, C.byref(first)),
                lib.perc_first_spanning_mixed(ctx.h, PL.BOND, None, 5, bp, 5, on_dev, C.byref(first)),
                lib.perc_first_spanning_mixed(ctx.h, PL.BOND, sp, 5, None, 5, on_dev, C.byref(first)),
                lib.perc_first_spanning_mixed(None, PL.BOND, sp, 5, bp, 5, on_dev, C.byref(first)),
            ]
            assert bad == [-1] * len(bad), (on_dev, bad)  # PERC_EINVAL
        # a refused call leaves the context usable
        ctx.occupy_device(PL.BOND, None, 0, db.data_ptr(), nb)
        assert ctx.label()["nspan"] > 0
    del ds, db


# ------------------------------------------------ 4. one context, many realisations
SEEDS6 = list(range(100, 106))
NONSPAN_AT = 2  # the third realisation is filled to p = 0.40 only


def test_one_context_reused_with_timing_is_fresh_untimed_contexts_occupy_random():
    """bench.py --occupancy device: perc_occupy_random on one timed context,
    against fresh untimed contexts given the host restatement of each order
    (perc_random_order)"""
    geom, p = CASES["S1"][:2]
    nb = api.nbonds(*geom)
    tbs = [int((0.40 if k == NONSPAN_AT else p) * nb) for k in range(len(SEEDS6))]
    stop = (1e-8, 10 ** 6)
    got = []
    with make_ctx("S1") as ctx:
        ctx.set_kernel_timing(True)
        for seed, tb in zip(SEEDS6, tbs):
            ctx.occupy_random(PL.BOND, 0, tb, seed)
            li = ctx.label()
            c = solve(ctx, stop) if li["nspan"] else ctx.conductance(tol=stop[0], itmax=stop[1])
            if li["nspan"]:
                check_family("S1", ctx)
            got.append((li, c))
        st = ctx.kernel_stats(reset=True)
    its = [c["iter"] for li, c in got if li["nspan"]]
    check_stats("S1", st, its, sum(c["t_solve_ms"] for li, c in got))
    for k, (seed, tb) in enumerate(zip(SEEDS6, tbs)):
        order = api.random_order(nb, tb, seed)
        with make_ctx("S1") as ctx:
            ctx.occupy(PL.BOND, bond_order=order, nbonds_=tb)
            li = ctx.label()
            assert (li["nspan"] > 0) == (k != NONSPAN_AT), (k, li)
            assert li == got[k][0], (k, li, got[k][0])
            if li["nspan"]:
                assert_same_solve(solve(ctx, stop), got[k][1], k)
            else:
                c = got[k][1]
                assert c["status"] == 1 and c["iter"] == 0 and c["gtop"] == 0.0 and c["gbot"] == 0.0, c


def test_one_context_reused_with_timing_is_fresh_untimed_contexts_device_orders():
    """bench.py --occupancy reference: perc_bondc_realisation(on_device=1) on
    one timed context, six orders in a row, the third not spanning"""
    geom, p = CASES["S1"][:2]
    nb = api.nbonds(*geom)
    tbs = [int((0.40 if k == NONSPAN_AT else p) * nb) for k in range(len(SEEDS6))]
    orders = [api.shuffled_ids(nb, s) for s in SEEDS6]
    d_orders = [dev(o) for o in orders]
    with make_ctx("S1") as ctx:
        ctx.set_kernel_timing(True)
        got = [ctx.bondc_realisation(None, tb, tol=1e-8, itmax=10 ** 6, device_ptr=d.data_ptr())
               for d, tb in zip(d_orders, tbs)]
        st = ctx.kernel_stats(reset=True)
    check_stats("S1", st, [r["iter"] for r in got if r["nspan"]], sum(r["t_solve_ms"] for r in got))
    for k, (o, tb) in enumerate(zip(orders, tbs)):
        with make_ctx("S1") as ctx:
            fresh = ctx.bondc_realisation(o, tb, tol=1e-8, itmax=10 ** 6)
            if k != NONSPAN_AT:
                check_family("S1", ctx)
        assert (fresh["nspan"] > 0) == (k != NONSPAN_AT), (k, fresh)
        assert fresh["status"] == (1 if k == NONSPAN_AT else 0), (k, fresh)
        assert_same_realisation(got[k], fresh, k)
    del d_orders


# ------------------------------------------------ 5. contexts in flight
SEEDS12 = list(range(100, 112))
_SERIAL = {}


def serial_realisations(tag):
    """the twelve realisations of the case on one serial untimed context
    (computed once)"""
    if tag not in _SERIAL:
        geom, p = CASES[tag][:2]
        nb = api.nbonds(*geom)
        tb = int(p * nb)
        orders = [api.shuffled_ids(nb, s) for s in SEEDS12]
        with make_ctx(tag) as ctx:
            res = [ctx.bondc_realisation(o, tb, tol=1e-8, itmax=10 ** 6) for o in orders]
            check_family(tag, ctx)
        assert all(r["nspan"] > 0 and r["status"] == 0 for r in res), [r["nspan"] for r in res]
        _SERIAL[tag] = (orders, tb, res)
    return _SERIAL[tag]


@pytest.mark.parametrize("tag,K", [("S3", 2), ("S3", 4), ("W", 4)])
def test_contexts_in_flight_return_the_serial_results(tag, K):
    """K contexts, one host thread each (ctypes drops the GIL inside libperc),
    timing on, device-resident orders: lane c runs realisations c, c + K,
    c + 2 K"""
    orders, tb, serial = serial_realisations(tag)
    lanes = [[c + j * K for j in range(3)] for c in range(K)]
    d_orders = {r: dev(orders[r]) for lane in lanes for r in lane}
    ctxs = [make_ctx(tag) for _ in range(K)]
    try:
        for c in ctxs:
            c.set_kernel_timing(True)
            c.kernel_stats(reset=True)

        def run(ci):
            out = [ctxs[ci].bondc_realisation(None, tb, tol=1e-8, itmax=10 ** 6, device_ptr=d_orders[r].data_ptr())
                   for r in lanes[ci]]
            return out, PL.lib().perc_last_error().decode(errors="replace")

        with ThreadPoolExecutor(K) as pool:
            per = [f.result() for f in [pool.submit(run, ci) for ci in range(K)]]
        for ci in range(K):
            res, last_error = per[ci]
            assert last_error == "ok", (ci, last_error)  # (thread-local: this lane's calls only)
            for r, got in zip(lanes[ci], res):
                print(tag, K, "lane", ci, "realisation", r, got["iter"], got["gtop"], serial[r]["gtop"])
                for k in ("nspan", "span_root", "iter"):
                    assert got[k] == serial[r][k], (ci, r, k, got[k], serial[r][k])
                for k in ("err", "gtop", "gbot"):
                    assert same_bits(got[k], serial[r][k]), (ci, r, k, got[k], serial[r][k])
            check_family(tag, ctxs[ci])
            check_stats(tag, ctxs[ci].kernel_stats(reset=True), [g["iter"] for g in res],
                        sum(g["t_solve_ms"] for g in res))
    finally:
        for c in ctxs:
            c.close()
    del d_orders


# ------------------------------------------------ 6. the benchmark itself
BENCH_MASTER = 58302  # bench.py's default --master
BENCH_L, BENCH_P = 128, 0.60
ASSOC_X = 1.5  # test_config_goldens.py: bar = ASSOC_X x the oracle's own association spread


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def test_bench_timed_step_is_the_api_on_a_fresh_untimed_context(tmp_path):
    """bench.py --gpus 1 --L 128 --steps 1 --warmup 1: one rank, so trial
    index k runs realisation k (ensemble.trial_indices: k * world + rank);
    the warmup is k = 0 and the timed step k = 1, drawn on the device from
    tseed(2) = api.trial_seeds(master, 1000)[1] (--occupancy device) at
    int(p * nb) bonds, solved with tol 1e-8 and itmax 10^6."""
    geom = (0, BENCH_L, BENCH_L, 0)
    nb = api.nbonds(*geom)
    tb = int(BENCH_P * nb)
    seed = int(api.trial_seeds(BENCH_MASTER, 1000)[1])
    order = api.random_order(nb, tb, seed)
    ref = api.replay_labels(*geom, PL.BOND, bond_order=order, nbond=tb)
    assert ref["perccln"] > 0  # it spans (CPU)
    d = str(tmp_path / "dump")
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--L", str(BENCH_L),
                        "--steps", "1", "--warmup", "1", "--dump-outputs", d],
                       capture_output=True, text=True, timeout=300, cwd=REPO, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    got = {n: np.load(os.path.join(d, n + ".npy")) for n in ("gtop", "gbot", "iter", "nspan")}
    assert all(a.dtype == np.float64 and a.shape == (1,) for a in got.values())
    with api.Context(*geom) as ctx:
        ctx.occupy_random(PL.BOND, 0, tb, seed)
        li = ctx.label()
        c = ctx.conductance(PL.RULE_BOND, PL.CUR_FORTRAN, tol=1e-8, itmax=10 ** 6)
    print("bench", got, li, c)
    assert li["nspan"] > 0 and got["nspan"][0] == li["nspan"]
    assert got["iter"][0] == c["iter"] > 50
    assert same_bits(got["gtop"], c["gtop"]) and same_bits(got["gbot"], c["gbot"]), (got, c)
    # the oracle's linbcg on that occupancy, and how far its own Gtop moves
    # when only the association of its dot products changes (descending and
    # tree sums: oracle_lib.conductance_decades)
    b1, b2 = api.bond_list(*geom)
    gval = O.f64(nb)
    O.lib().or_bond_values(0, nb, b1, b2, ref["bond_label"], O.i32(1), ref["perccln"], 1.0, 1e-12, gval)
    lit = O.conductance_decades(*geom, b1, b2, gval, [1e-8], itmax=10 ** 6, dot_order=0)[0][0]
    spread = max(rel(O.conductance_decades(*geom, b1, b2, gval, [1e-8], itmax=10 ** 6, dot_order=k)[0][0]["gtop"],
                     lit["gtop"]) for k in (1, 2))
    bar = max(1e-10, ASSOC_X * spread)
    print("bench oracle", lit["gtop"], lit["iter"], "spread", spread, "bar", bar, "rel", rel(c["gtop"], lit["gtop"]))
    assert rel(c["gtop"], lit["gtop"]) <= bar, (c["gtop"], lit["gtop"], spread, bar)
