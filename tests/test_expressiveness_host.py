"""Colour refinement on the host (csrc/wl_refine.cpp through desco_amd/expressiveness.py): the twin's bits against the
definition restated in Python, its partition against an exact tuple-colour refinement (tests/wl_reference.py), the named
pairs a family cannot tell apart, the invariances, the error floor and the refusals."""
import math

import numpy as np
import pytest

import wl_reference as R
from desco_amd import _lib, expressiveness as X
from desco_amd.batch import GraphBatch
from desco_amd.graphs import GraphSet
from desco_amd.partition import build_partition


def small_block(anchored=True):
    """Three neighborhoods by hand on the 4-slot layout: a triangle with a tail (slots 0 / 1 among the count rows, 2 / 3
    from the anchor, an EMPTY slot in most rows), a neighborhood with NO count rows, and a path."""
    edges = {   # (destination row, slot) -> sources; rows 0..3 and 4..5 are count rows, 6..8 the anchors
        (0, 0): [1], (1, 0): [0], (0, 2): [6], (1, 2): [6], (1, 1): [2], (2, 1): [1, 3], (3, 1): [2],
        (6, 0): [0, 1],
        (4, 1): [5], (5, 1): [4], (5, 3): [8], (8, 1): [5],
    }
    num_rows, slots = 9, 4
    vrowptr, vcol = [0], []
    for v in range(num_rows * slots):
        vcol += edges.get((v // slots, v % slots), [])
        vrowptr.append(len(vcol))
    seg_ptr = [0, 4, 4, 6]
    if not anchored:                                     # the same rows as three anchor-free segments
        return X.Block(np.array(vrowptr, np.int32), np.array(vcol, np.int32), num_rows, slots,
                       np.array([0, 4, 6, 9], np.int32), -1)
    return X.Block(np.array(vrowptr, np.int32), np.array(vcol, np.int32), num_rows, slots, np.array(seg_ptr, np.int32), 6)


def unanchored_block():
    """the rows 0..3 and 4..5 of ``small_block`` without the entries that name an anchor"""
    b = small_block()
    vr, vc = b.vrowptr.tolist(), b.vcol.tolist()
    keep = [c < 6 for c in vc]
    new_vr = [0] + [sum(keep[:o]) for o in vr[1:6 * 4 + 1]]
    return X.Block(np.array(new_vr, np.int32), np.array([c for c, k in zip(vc, keep) if k], np.int32), 6, 4,
                   np.array([0, 4, 4, 6], np.int32), -1)


# ---- 1. bits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounds", [0, 1, 3, 64])
@pytest.mark.parametrize("view", ["shmp", "hetero", "plain", (1, 0, 0, 3)])
def test_twin_equals_the_definition_bit_for_bit(rounds, view):
    rng = np.random.default_rng(7)
    for b in (small_block(), unanchored_block()):
        for init in (None, rng.integers(-2 ** 63, 2 ** 63 - 1, size=b.num_rows, dtype=np.int64)):
            group = X.view_groups(view, 4)
            sig, colours, status = R.hash_refine(*R.block_args(b, group), rounds, init)
            got = X.refine(b, view, rounds, backend="host", init=init, keep_colours=True)
            assert X.last_backend == got.last_backend == "host"
            assert got.status.tolist() == status == [0, 0, 0]
            assert got.signature.tolist() == sig
            assert got.colours.tolist() == [0 if c is None else c for c in colours]
            one = X.refine(b, view, rounds, backend="host", init=init, num_threads=1)
            assert one.colours is None and np.array_equal(one.signature, got.signature)
    assert R.mix(0) == 0 and R.mix(R.G) != 0


def test_twin_equals_the_definition_on_two_slot_graphs():
    g = GraphSet.from_edge_lists(R.atlas_connected()[::97])
    b = X._block(GraphBatch(g, "cpu"))
    for view in ("plain", "shmp"):
        for rounds in (0, 1, 3):
            sig, colours, status = R.hash_refine(*R.block_args(b, X.view_groups(view, 2)), rounds)
            got = X.refine(GraphBatch(g, "cpu"), view, rounds, backend="host", keep_colours=True)
            assert got.signature.tolist() == sig and got.colours.tolist() == colours and not got.status.any()


# ---- 2. the partition equals exact refinement ------------------------------------------------------------------------------
def partitions_agree(b, view, rounds):
    group = X.view_groups(view, b.slots)
    exact = R.exact_refine(*R.block_args(b, group), rounds)
    got = X.refine(b, view, rounds, backend="host")
    assert not got.status.any()
    classes = X.classes_of(got.signature)
    assert R.partition_of(exact) == R.partition_of(got.signature.tolist()) == R.partition_of(classes.class_id.tolist())
    assert classes.num_classes == len(set(exact)) and int(classes.class_size.sum()) == len(exact)
    return classes.num_classes


@pytest.mark.parametrize("rounds", [0, 1, 2, 8])
def test_atlas_whole_graphs_partition_is_exact(rounds):
    b, views = R.blocks()["atlas/graphs"]
    counts = {view: partitions_agree(b, view, rounds) for view in views}
    print(f"[classes] atlas whole graphs, {rounds} rounds: {counts}")
    assert counts["plain"] <= counts["shmp"] <= 994
    if rounds == 0:
        assert counts == {"plain": 5, "shmp": 5}             # the node count is all that is left
    if rounds == 8:
        assert counts["shmp"] > counts["plain"]


@pytest.mark.parametrize("name", [k for k in ("atlas", "golden", "cox2", "syn")])
@pytest.mark.parametrize("definition", ["ball", "restricted"])
def test_neighborhood_partition_is_exact(name, definition):
    b, views = R.blocks()[f"{name}/{definition}"]
    assert views == ("plain", "hetero", "shmp")
    counts = {view: partitions_agree(b, view, 8) for view in views}
    print(f"[classes] {name}/{definition}, 8 rounds: {counts} of {len(b.seg_ptr) - 1} neighborhoods")
    assert counts["plain"] <= counts["hetero"] <= counts["shmp"]


@pytest.mark.parametrize("name", ["golden", "cox2", "syn"])
def test_other_whole_graphs_partition_is_exact(name):
    b, views = R.blocks()[f"{name}/graphs"]
    for view in views:
        partitions_agree(b, view, 8)
        partitions_agree(b, view, 2)


# ---- 3. the named pairs ----------------------------------------------------------------------------------------------------
def anchored_pair(pair):
    """(signatures per view, triangle truth) of the two anchored graphs: each graph relabelled so that its anchor is the
    largest id, whose canonical neighborhood is then the whole graph"""
    atlas = R.atlas_connected()
    graphs = [R.anchored_at_largest(atlas[i], a) for i, a in pair]
    part = build_partition(GraphSet.from_edge_lists(graphs), 4)
    mine = [k for k in range(part.num_neigh) if part.neigh_index[k, 1] == graphs[part.neigh_index[k, 0]][0] - 1]
    assert [int(part.neigh_index[k, 0]) for k in mine] == [0, 1]
    assert [int(part.count_ptr[k + 1] - part.count_ptr[k]) for k in mine] == [g[0] - 1 for g in graphs]
    sigs = {view: X.refine(part, view, 8, backend="host").signature[mine] for view in X.VIEWS}
    return sigs, np.array([[R.triangles(g)] for g in graphs], dtype=np.int64)


def floor_of_pair(sig, truth, space="log2"):
    return X.error_floor(X.classes_of(sig), truth, space)


def test_pair_that_only_the_triangle_split_separates():
    sigs, truth = anchored_pair(R.PAIR_PLAIN_BLIND)
    assert truth.tolist() == [[0], [2]]
    assert sigs["plain"][0] == sigs["plain"][1] and sigs["shmp"][0] != sigs["shmp"][1]
    f = floor_of_pair(sigs["plain"], truth)
    assert f.ambiguous_classes.tolist() == [1] and f.ambiguous_sets.tolist() == [2]
    assert f.sse_floor[0] == pytest.approx(math.log2(3) ** 2 / 2, rel=1e-14)      # y = 0 and log2 3 around their mean
    g = floor_of_pair(sigs["shmp"], truth)
    assert g.ambiguous_classes.tolist() == [0] and g.ambiguous_sets.tolist() == [0] and g.sse_floor[0] == 0.0
    assert floor_of_pair(sigs["plain"], truth, "count").sse_floor[0] == 2.0        # 0 and 2 around 1


def test_pair_that_no_view_separates():
    sigs, truth = anchored_pair(R.PAIR_SHMP_BLIND)
    assert truth.tolist() == [[6], [8]]
    for view in X.VIEWS:
        assert sigs[view][0] == sigs[view][1], view
        f = floor_of_pair(sigs[view], truth)
        assert f.ambiguous_classes.tolist() == [1] and f.ambiguous_sets.tolist() == [2]
        assert f.sse_floor[0] == pytest.approx((math.log2(9) - math.log2(7)) ** 2 / 2, rel=1e-12)
        assert f.mse_floor[0] == pytest.approx(f.sse_floor[0] / 2) and f.norm_mse_floor[0] == pytest.approx(1.0)


def test_whole_graph_pair_that_plain_merges():
    atlas = R.atlas_connected()
    graphs = [atlas[i] for i in R.PAIR_GRAPHS_PLAIN_BLIND]
    truth = np.array([[R.triangles(g)] for g in graphs], dtype=np.int64)
    assert truth.tolist() == [[0], [2]]
    c = X.graph_classes(GraphSet.from_edge_lists(graphs), 8, "plain", backend="host")
    assert c.num_classes == 1 and c.class_id.tolist() == [0, 0] and c.neigh_index is None
    f = X.error_floor(c, truth)
    assert f.ambiguous_sets.tolist() == [2] and f.sse_floor[0] == pytest.approx(math.log2(3) ** 2 / 2, rel=1e-14)
    assert X.graph_classes(GraphSet.from_edge_lists(graphs), 8, "shmp", backend="host").num_classes == 2


# ---- 4. invariances, bit for bit -------------------------------------------------------------------------------------------
def test_row_order_slices_and_selections_leave_the_signatures_alone():
    g = R.graph_sets()["cox2"]
    part = build_partition(g, 4)
    for view in X.VIEWS:
        whole = X.refine(part, view, 8, backend="host").signature
        assert np.array_equal(X.refine(part.degree_sorted(), view, 8, backend="host").signature, whole)
        assert np.array_equal(X.refine(part.slice(100, 700), view, 8, backend="host").signature, whole[100:700])
        idx = np.arange(3, part.num_neigh, 7)
        assert np.array_equal(X.refine(part.select(idx), view, 8, backend="host").signature, whole[idx])
    by_name = X.neighborhood_classes(g, 4, 8, "shmp", backend="host")
    assert np.array_equal(by_name.signature, X.refine(part, "shmp", 8, backend="host").signature)
    assert np.array_equal(by_name.neigh_index, part.neigh_index) and X.last_backend == "host"


def test_more_rounds_and_finer_views_refine():
    b, _ = R.blocks()["atlas/ball"]
    sig = {(v, r): X.refine(b, v, r, backend="host").signature.tolist() for v in X.VIEWS for r in range(5)}
    for v in X.VIEWS:
        for r in range(4):
            assert R.refines(sig[v, r + 1], sig[v, r]), (v, r)
    for r in range(5):
        assert R.refines(sig["shmp", r], sig["hetero", r]) and R.refines(sig["hetero", r], sig["plain", r]), r
    assert len(set(sig["plain", 4])) > len(set(sig["plain", 1])) > len(set(sig["plain", 0]))


# ---- 5. error_floor --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", ["log2", "count"])
def test_error_floor_equals_a_loop_over_classes(space):
    rng = np.random.default_rng(3)
    S, Q = 400, 5
    classes = X.classes_of(rng.integers(0, 60, size=S).astype(np.int64) * 7919 - 200000)
    truth = rng.integers(0, 4, size=(S, Q)).astype(np.int64) * rng.integers(0, 2, size=(S, Q))
    truth[:, 4] = classes.class_id % 3                                   # a column that no class is ambiguous in
    f = X.error_floor(classes, truth, space)
    for q in range(Q):
        amb_c = amb_s = 0
        sse = 0.0
        for c in range(classes.num_classes):
            t = truth[classes.class_id == c, q]
            y = np.log2(1.0 + t) if space == "log2" else t.astype(np.float64)
            if len(set(t.tolist())) > 1:
                amb_c, amb_s = amb_c + 1, amb_s + len(t)
                sse += float(((y - y.mean()) ** 2).sum())
        assert (int(f.ambiguous_classes[q]), int(f.ambiguous_sets[q])) == (amb_c, amb_s)
        assert f.sse_floor[q] == pytest.approx(sse, rel=1e-12)
        y = np.log2(1.0 + truth[:, q]) if space == "log2" else truth[:, q].astype(np.float64)
        assert f.mse_floor[q] == pytest.approx(sse / S, rel=1e-12)
        assert f.norm_mse_floor[q] == pytest.approx(sse / S / np.var(y), rel=1e-12)
    assert f.ambiguous_classes[4] == 0 and f.sse_floor[4] == 0.0 and f.mse_floor[4] == 0.0 and f.norm_mse_floor[4] == 0.0
    assert f.ambiguous_classes[0] > 0 and f.sse_floor[0] > 0
    rows = f.table(names=list("abcde"))
    assert [r["query"] for r in rows] == list("abcde") and rows[0]["ambiguous_sets"] == int(f.ambiguous_sets[0])
    assert set(rows[0]) == {"query", "ambiguous_sets", "ambiguous_classes", "sse_floor", "mse_floor", "norm_mse_floor"}
    with pytest.raises(ValueError, match="space"):
        X.error_floor(classes, truth, "ln")


def test_error_floor_on_exact_ground_truth():
    """The whole route on a data set: the classes of a cox2-shaped slice and the exact canonical counts at their nodes."""
    from helpers import standard_queries
    g = R.graph_sets()["cox2"]
    queries = standard_queries()[1][:6]
    coarse, fine = (X.neighborhood_classes(g, 4, r, "shmp", backend="host") for r in (1, 8))
    truth = X.neighborhood_truth(g, fine, queries, backend="host")
    assert truth.shape == (fine.num_sets, 6) and truth.dtype == np.int64 and truth.max() > 0
    f1, f8 = X.error_floor(coarse, truth), X.error_floor(fine, truth)
    assert (f8.sse_floor <= f1.sse_floor + 1e-9).all() and (f8.ambiguous_sets <= f1.ambiguous_sets).all()
    assert f1.ambiguous_sets.max() > 0
    gt = X.graph_truth(g, queries, backend="host")
    assert gt.shape == (g.num_graphs, 6) and (gt.sum(axis=0) >= truth.sum(axis=0)).all()


# ---- 6. refusals by name -----------------------------------------------------------------------------------------------------
def test_refusals_name_what_is_wrong():
    b = small_block()
    with pytest.raises(ValueError, match="rounds = 65.*DESCO_WL_MAX_ROUNDS"):
        X.refine(b, "shmp", 65, backend="host")
    with pytest.raises(RuntimeError, match="desco_wl_refine: a group entry"):
        X.refine(b, (0, 1, 4, 0), 1, backend="host")
    with pytest.raises(ValueError, match="hetero.*whole graphs"):
        X.refine(GraphBatch(GraphSet.from_edge_lists(R.atlas_connected()[:3]), "cpu"), "hetero", 1, backend="host")
    with pytest.raises(ValueError, match="hetero"):
        X.graph_classes(GraphSet.from_edge_lists(R.atlas_connected()[:3]), 8, "hetero", backend="host")
    with pytest.raises(ValueError, match="unknown view"):
        X.refine(b, "wl", 1, backend="host")
    with pytest.raises(ValueError, match="unknown backend"):
        X.refine(b, "shmp", 1, backend="gpu")

    L = _lib.lib()
    vr, vc, sp = b.vrowptr, b.vcol, b.seg_ptr
    grp = np.arange(4, dtype=np.int32)
    sig, status = np.zeros(3, np.int64), np.zeros(3, np.int32)

    def call(vrowptr=vr.ctypes.data, slots=4, group=grp.ctypes.data, seg_ptr=sp.ctypes.data, rounds=8,
             sig_=sig.ctypes.data, status_=status.ctypes.data, segs=3):
        return L.desco_wl_refine(vrowptr, vc.ctypes.data, 9, slots, group, seg_ptr, segs, 6, None, rounds, 0, sig_, None,
                                 status_)

    def rejects(rc, word):
        assert rc == -1
        msg = L.desco_last_error()
        assert b"desco_wl_refine" in msg and word in msg, msg
        assert L.desco_rng_next(None, None, None) == -1          # (resets the message for the next case)

    assert call() == 0
    rejects(call(rounds=65), b"rounds")
    rejects(call(rounds=-1), b"rounds")
    rejects(call(slots=0), b"slots")
    rejects(call(slots=5), b"slots")
    rejects(call(group=np.array([0, 1, 2, 4], np.int32).ctypes.data), b"group entry")
    rejects(call(group=None), b"group is null")
    rejects(call(vrowptr=None), b"vrowptr is null")
    rejects(call(seg_ptr=None), b"seg_ptr is null")
    rejects(call(sig_=None), b"sig is null")
    rejects(call(status_=None), b"status is null")
    rejects(call(segs=-1), b"negative")


def test_an_entry_outside_its_segment_is_guarded():
    b = small_block()
    want = X.refine(b, "shmp", 3, backend="host", keep_colours=True)
    vc = b.vcol.copy()
    at = int(b.vrowptr[4 * 4 + 1])                      # row 4, slot 1: source 5 of the third neighborhood ...
    assert vc[at] == 5
    vc[at] = 2                                          # ... now names a row of the first
    got = X.refine(b._replace(vcol=vc), "shmp", 3, backend="host", keep_colours=True)
    assert got.status.tolist() == [0, 0, -1]
    assert np.array_equal(got.signature[:2], want.signature[:2]) and got.signature[2] == 0
    mine = np.array([4, 5, 8])
    assert (got.colours[mine] == 0).all() and np.array_equal(np.delete(got.colours, mine), np.delete(want.colours, mine))
    vc[at] = 7                                          # another neighborhood's anchor is outside as well
    assert X.refine(b._replace(vcol=vc), "shmp", 3, backend="host").status.tolist() == [0, 0, -1]
    with pytest.raises(RuntimeError, match="not refined"):
        X._require_refined(got, "test")


# ---- the driver --------------------------------------------------------------------------------------------------------------
def test_driver_writes_its_table(tmp_path, capsys):
    import csv
    import importlib.util
    import os
    import warnings
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("expressiveness_driver", os.path.join(root, "expressiveness.py"))
    driver = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(driver)
    argv = ["--datasets", "MUTAG", "--graphs", "--backend", "host", "--query_size", "3", "4", "--rounds", "1",
            "--output_dir", str(tmp_path), "--data_root", str(tmp_path / "none")]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                  # (the stand-in set announces itself)
        first, second = driver.main(argv), driver.main(argv + ["--views", "plain", "--no-restricted"])
    assert os.path.basename(first) == "expressiveness_0.csv" and os.path.basename(second) == "expressiveness_1.csv"
    rows = list(csv.reader(open(first)))
    assert rows[0][1:7] == ["dataset", "level", "view", "rounds", "sets", "classes"]
    assert rows[0][7:11] == ["ambiguous_sets_6", "ambiguous_classes_6", "mse_floor_6", "norm_mse_floor_6"]
    assert len(rows[0]) == 7 + 4 * 8                                     # the 8 connected patterns of 3 and 4 nodes
    assert [(r[2], r[3]) for r in rows[1:]] == [("neighborhood/restricted", "plain"), ("neighborhood", "hetero"),
                                                ("neighborhood", "shmp"), ("graph", "plain"), ("graph", "shmp")]
    assert all(int(r[5]) >= int(r[6]) > 1 for r in rows[1:])
    assert [r[2] for r in list(csv.reader(open(second)))[1:]] == ["neighborhood", "graph"]
    assert "norm_mse_floor" in capsys.readouterr().out
