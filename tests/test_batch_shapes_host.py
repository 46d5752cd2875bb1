"""tests/batch_shapes.py on the host (no device): every support predicate
returns what the shape table says, per kind, the refused neighbours included,
and the item selection gives every supported (shape, kind) what the GPU tests
of test_batch_shapes.py stand on -- a partial occupancy exactly one cluster
spans -- plus several spanning clusters on flat shapes and none on thin ones."""
import pytest

import batch_shapes as BS
from percolation_amd import _lib as L
from percolation_amd import api

FAMILIES = [("cond", api.batch_cond_supported, "perc_batch_cond_supported"),
            ("large", api.batch_large_supported, "perc_batch_large_supported"),
            ("weighted", api.batch_weighted_supported, "perc_batch_weighted_supported"),
            ("currents", api.batch_currents_supported, "perc_batch_currents_supported")]
ROW_IDS = [BS.lat_id(r.lat) for r in BS.TABLE]


@pytest.mark.parametrize("row", BS.TABLE, ids=ROW_IDS)
def test_predicates_return_the_table(row):
    for name, f, symbol in FAMILIES:
        raw = getattr(L.lib(), symbol)
        for kind in BS.KINDS:
            want = kind in getattr(row, name)
            assert f(kind, *row.lat) is want, (name, BS.KIND_NAME[kind], row.lat)
            assert raw(kind, *row.lat) == (1 if want else 0), (name, BS.KIND_NAME[kind], row.lat)
    assert api.batch_supported(*row.lat) is (L.BOND in row.cond), row.lat
    assert api.scan_supported(*row.lat) is row.scan, row.lat
    for nexact in (0, 12, 1024):
        assert api.batch_clusters_supported(*row.lat, nexact) is row.clusters, (row.lat, nexact)


def test_table_is_the_issues():
    """the rows that pin a boundary, by what makes them one"""
    N = {lat: BS.sizes(lat)[0] for lat in BS.ROW}
    assert (N[0, 64, 34, 0], N[0, 64, 35, 0], N[0, 64, 66, 0], N[0, 64, 67, 0]) == (2048, 2112, 4096, 4160)
    assert (N[0, 3, 2732, 0], N[0, 3, 2733, 0]) == (8190, 8193)
    assert N[0, 4096, 3, 0] == 4096 and N[1, 2048, 3, 1] == 2048 and N[0, 2048, 4, 0] == 4096
    t = {lat: BS.sizes(lat)[1] for lat in BS.ROW}
    assert t[0, 3, 5461, 0] == t[0, 5461, 3, 0] == 16383 and t[0, 3, 5462, 0] == 16386
    assert t[0, 256, 64, 0] == t[0, 1024, 16, 0] == t[1, 4, 4096, 1] == t[0, 4096, 4, 0] == 16384
    # the refused neighbours the GPU tests call
    assert BS.ROW[0, 4500, 3, 0].cond == BS.BOND_ONLY and BS.ROW[0, 4096, 3, 0].cond == BS.ALL
    assert not BS.ROW[0, 3, 2733, 0].cond and BS.ROW[0, 3, 2732, 0].cond == BS.ALL
    assert not BS.ROW[0, 50, 72, 0].weighted and BS.ROW[0, 50, 71, 0].weighted == BS.ALL
    assert not BS.ROW[1, 50, 52, 0].weighted and BS.ROW[1, 50, 51, 0].weighted == BS.ALL
    assert not BS.ROW[0, 3, 5462, 0].scan and BS.ROW[0, 3, 5461, 0].scan
    for lat in BS.TINY + BS.THIN + BS.FLAT + BS.LONG:
        assert lat in BS.ROW


def runs(row):
    """the kinds any kernel takes on a shape"""
    any_cond = row.cond | row.large | row.weighted | row.currents
    return [k for k in BS.KINDS if k in any_cond or row.scan or row.clusters]


@pytest.mark.parametrize("row", [r for r in BS.TABLE if runs(r)], ids=[BS.lat_id(r.lat) for r in BS.TABLE if runs(r)])
def test_selection_has_a_partial_single_spanning_item(row):
    for kind in runs(row):
        g = BS.grid(row.lat, kind)
        once = [x for x in g if x[3] == 1]
        assert once, (row.lat, BS.KIND_NAME[kind], g)
        f, ns, nbc, _ = once[0]
        _, t, nb = BS.sizes(row.lat)
        # (f <= 0.98 but for 5461 x 3 site and mixed and 4500 x 3 mixed: 0.995)
        assert f in BS.FRACTIONS and ns <= t and nbc <= nb and (ns < t or nbc < nb)
        sel = BS.select(row.lat, kind)
        assert sel["single"] == (ns, nbc) and BS.nspan_host(row.lat, kind, *sel["single"]) == 1
        # the full lattice is one cluster, with the spill slot or without
        assert BS.nspan_host(row.lat, kind, *sel["full"]) == BS.nspan_host(row.lat, kind, *sel["spill"]) == 1
        for name, ok in (("none", lambda s: s == 0), ("multi", lambda s: s > 1)):
            if name in sel:
                assert ok(BS.nspan_host(row.lat, kind, *sel[name])), (row.lat, kind, name)


def having(shapes, name):
    return [lat for lat in shapes if any(name in BS.select(lat, k) for k in BS.KINDS)]


def test_flat_shapes_give_several_spanning_clusters():
    got = having(BS.FLAT, "multi")
    print("flat shapes with an nspan > 1 item:", got)
    assert len(got) >= 3


def test_thin_shapes_give_items_nothing_spans():
    got = having(BS.THIN, "none")
    print("thin shapes with an nspan == 0 item:", got)
    assert len(got) >= 3
