"""GPU labeling of structured occupancies (label_patterns.py) against the
oracle's replays: the inputs uniform percolation never produces.

Rows that are one run from edge to edge (k_cc_tile_w's ballots, the carry
from column 63 to 64, hundreds of lanes skipping their union), stripes and
combs whose crossing links all join different clusters (the merges'
deduplication by parent pair), serpentines and spirals where every hook
lengthens one chain (the merges' CAS retries, the cluster count as member
roots minus hooks), 64 / 65 / 150 / 1025 spanning clusters (k_span_top's
root list and its K = 3 flags per thread), and -- one context per test, the
patterns one after the other -- every transition of "the previous labeling
spanned" that decides whether k_cc_compress_spec runs.  What the oracle's
partitions are is pinned on the CPU by test_label_patterns_host.py.
"""
import numpy as np
import pytest

import label_patterns as LP
import oracle_lib as O
from percolation_amd import api
from test_gpu_parity import REL, rel
from test_label_patterns_host import KIND, reused_oracle
from test_labeling_oracle import check

# many-span, one-span and none-span cases in turn (as they are on the open
# square lattice; elsewhere the oracle says what they are)
SEQ = {
    "bond": ["vstripes", "serp", "hstripes", "combs_joined", "combs", "vstripes", "serp_short",
             "hstripes_rungs", "vserp", "vstripes", "stair", "spiral", "hstripes", "serp"],
    "site": ["vstripes", "serp", "hstripes", "combs_joined", "combs", "vstripes", "serp_short",
             "checker", "serp", "vstripes", "combs_joined"],
    "mixed": ["s:vstripes", "b:serp", "s:hstripes", "s:combs_joined", "b:combs", "b:vstripes",
              "s:serp_short", "b:hstripes_rungs", "s:vstripes*b:vstripes", "s:serp", "b:hstripes",
              "b:combs_joined", "s:combs", "b:vserp", "b:serp_short", "s:checker", "b:spiral",
              "b:stair", "s:vstripes"],
}
SAME = ("nspan", "span_root", "span_sites", "nclusters")


def occupy(ctx, kind_name, so, bo):
    ctx.occupy(KIND[kind_name], site_order=so, nsites=0 if so is None else len(so), bond_order=bo,
               nbonds_=0 if bo is None else len(bo))


def label_and_check(ctx, kind_name, geom, name, order, so, bo):
    """one ordered occupancy through perc_label and everything read off it"""
    lat, m, n, pbc = geom
    tag = "%s (%s order)" % (name, order)
    occupy(ctx, kind_name, so, bo)
    li = ctx.label(canon=True)
    try:
        check(li, *reused_oracle(kind_name, lat, m, n, pbc, so, bo))
    except AssertionError as e:
        raise AssertionError("%s: %s" % (tag, e)) from None
    on = LP.oracle_numbers(kind_name, lat, m, n, pbc, so, bo)
    roots = LP.spanning_roots(on["canon"], m, n)
    # the exact number of spanning clusters, past the 64 the list keeps too
    assert li["nspan"] == len(roots), (tag, li["nspan"], len(roots))
    if len(roots):
        want = int(np.count_nonzero(on["canon"] == li["span_root"]))
        assert li["span_sites"] == want, (tag, li["span_sites"], want)
    else:
        assert (li["span_root"], li["span_sites"]) == (0, 0), (tag, li)
    if len(roots) > 1:  # the lowest-label rule reads the host order
        assert li["replayed"] == 1, tag
        assert li["perccln"] == on["perccln"], (tag, li["perccln"], on["perccln"])
        assert li["span_root"] == on["span_root"], (tag, li["span_root"], on["span_root"])
    else:
        assert li["replayed"] == 0, tag
    if kind_name != "mixed":
        want = (on["maxcs"], int(on["csize"][on["perccln"]]) if on["perccln"] else 0)
        assert ctx.cluster_sizes() == want, (tag, ctx.cluster_sizes(), want)
    ln = ctx.label_numbers(KIND[kind_name])
    for key in ("bond_label", "site_label"):
        if on[key] is not None:
            assert np.array_equal(ln[key], on[key]), (tag, key)
    assert ln["perccln"] == on["perccln"], (tag, ln["perccln"], on["perccln"])
    # the same occupancy labelled again (now behind a labeling of its own
    # spanning verdict), without and with the canonical labels
    l2 = ctx.label()
    l3 = ctx.label(canon=True)
    for key in SAME:
        assert li[key] == l2[key] == l3[key], (tag, key, li[key], l2[key], l3[key])
    assert np.array_equal(l3["canon"], li["canon"]), tag
    return len(roots)


@pytest.mark.gpu
@pytest.mark.parametrize("geom", LP.GEOMS)
@pytest.mark.parametrize("kind_name", LP.KINDS)
def test_patterns_vs_oracle(geom, kind_name):
    lat, m, n, pbc = geom
    cases = {name: (sids, bids) for name, sids, bids in LP.cases(kind_name, lat, m, n, pbc)}
    assert set(SEQ[kind_name]) == set(cases)  # (every pattern runs)
    seen = set()
    with api.Context(lat, m, n, pbc) as ctx:
        for i, name in enumerate(SEQ[kind_name]):
            sids, bids = cases[name]
            orders = [LP.ORDERS[i % 3]]
            k = 0
            while k < len(orders):
                order = orders[k]
                so = None if sids is None else LP.ordered(sids, order, 100 + i)
                bo = None if bids is None else LP.ordered(bids, order, 200 + i)
                nspan = label_and_check(ctx, kind_name, geom, name, order, so, bo)
                if nspan > 1 and len(orders) == 1:  # several span: all three orders
                    orders += [o for o in LP.ORDERS if o != order]
                k += 1
            seen.add(min(nspan, 2))
    if lat == 0 and not pbc:
        assert seen == {0, 1, 2}  # (none, one and many spanning clusters were all met)


@pytest.mark.gpu
def test_stripes_conductance_uses_the_lowest_label():
    """Bond stripes, the one place where a wrong label changes a number that
    can be stated: 70 spanning clusters occupied from the highest bond id
    down, so the lowest reference label is not the lowest root; only that
    stripe gets g0 (hazard H4)."""
    lat, m, n, pbc = 0, 140, 12, 0
    bo = LP.ordered(LP.bond_ids("vstripes", lat, m, n, pbc), "desc")
    on = LP.oracle_numbers("bond", lat, m, n, pbc, None, bo)
    roots = LP.spanning_roots(on["canon"], m, n)
    assert len(roots) == 70 and on["span_root"] != roots[0]
    with api.Context(lat, m, n, pbc) as ctx:
        occupy(ctx, "bond", None, bo)
        li = ctx.label()
        assert li["nspan"] == 70 and li["replayed"] == 1 and li["perccln"] == on["perccln"]
        assert li["span_root"] == on["span_root"]
        c = ctx.conductance(tol=1e-14, itmax=100000)
    b1, b2 = LP.bonds(lat, m, n, pbc)[:2]
    nb = len(b1)
    gval = O.f64(nb)
    O.lib().or_bond_values(0, nb, b1, b2, on["bond_label"], O.i32(1), on["perccln"], 1.0, 1e-12, gval)
    oc = O.conductance(lat, m, n, pbc, b1, b2, gval, tol=1e-14, itmax=100000)
    assert oc["gtop"] > 0.05  # (a chain of n - 1 = 11 unit bonds)
    assert rel(c["gtop"], oc["gtop"]) < REL, (c["gtop"], oc["gtop"])
