"""Exact NON-INDUCED ground truth on the host: count[v][q] = #{injective f : f sends every edge of q onto an edge of G,
max(im f) = v} / |Aut(q)|.  The matcher's non-induced mode against networkx VF2 monomorphisms (groundtruth_mono_vf2.py),
the census + transform route against the matcher, closed forms, the unchanged defaults, caching and refusals.
Integers, bit-exact."""
import math

import networkx as nx
import numpy as np
import pytest
import torch

import groundtruth_labelled_vf2 as LV
import groundtruth_mono_vf2 as M
import groundtruth_vf2 as V
from desco_amd import _lib, groundtruth
from desco_amd.graphs import GraphSet
from desco_amd.groundtruth import (canonical_counts, canonical_counts_labelled, canonical_counts_match,
                                   canonical_counts_match_labelled, census_classes, match_plan, match_plan_labelled,
                                   noninduced_matrix)
from helpers import golden_graphs, random_family_graphs, standard_queries

TRIANGLE = [(3, [(0, 1), (1, 2), (0, 2)])]


def _class_index(k, g):
    hits = [i for i, (n, e) in enumerate(census_classes(k)) if nx.is_isomorphic(V.to_nx(n, e), g)]
    assert len(hits) == 1
    return hits[0]


def test_the_flag_is_honoured_on_one_triangle():
    gs = GraphSet.from_edge_lists(TRIANGLE)
    p3 = nx.path_graph(3)
    for kw in (dict(), dict(method="matcher")):
        assert canonical_counts(gs, [p3], backend="host", **kw).reshape(-1).tolist() == [0, 0, 0]
        assert canonical_counts(gs, [p3], backend="host", induced=True, **kw).reshape(-1).tolist() == [0, 0, 0]
        assert canonical_counts(gs, [p3], backend="host", induced=False, **kw).reshape(-1).tolist() == [0, 0, 3]
    assert canonical_counts_match(gs, [p3], backend="host").reshape(-1).tolist() == [0, 0, 0]
    assert canonical_counts_match(gs, [p3], backend="host", induced=False).reshape(-1).tolist() == [0, 0, 3]
    assert canonical_counts(gs, [p3], backend="vf2").reshape(-1).tolist() == [0, 0, 0]
    assert canonical_counts(gs, [p3], backend="vf2", induced=False).reshape(-1).tolist() == [0, 0, 3]


@pytest.mark.parametrize("which", ["sparse", "dense"])
def test_host_matcher_equals_vf2_monomorphisms(which):
    graphs, queries, want = M.yardstick(which)
    assert len(queries) == 34 and sum(n for n, _ in graphs) == (433 if which == "sparse" else 18)
    totals = want.sum(axis=0)
    assert (totals > 0).sum() >= (23 if which == "sparse" else 28), totals.tolist()     # (on the VF2 side alone)
    gs = GraphSet.from_edge_lists(graphs)
    got = canonical_counts_match(gs, queries, backend="host", induced=False)
    assert got.dtype == torch.double and got.shape == want.shape
    assert got.long().tolist() == want.tolist()
    # the public entry: 3..5 nodes through the census, 7 nodes through the matcher, joined in query order
    assert canonical_counts(gs, queries, backend="host", induced=False).long().tolist() == want.tolist()
    induced = canonical_counts(gs, queries, backend="host").long()
    assert (torch.from_numpy(want) >= induced).all() and (torch.from_numpy(want) > induced).any()
    if which == "dense":                                # the package's own vf2 backend is the same procedure
        sel = [0, 5, 33]
        assert canonical_counts(gs, [queries[i] for i in sel], backend="vf2",
                                induced=False).long().tolist() == want[:, sel].tolist()


def test_transform_entries_in_k4_k5_and_k3():
    m4, m5, m3 = noninduced_matrix(4), noninduced_matrix(5), noninduced_matrix(3)
    k4, k5, k3 = (_class_index(k, nx.complete_graph(k)) for k in (4, 5, 3))
    paw = nx.Graph([(0, 1), (1, 2), (2, 0), (2, 3)])
    diamond = nx.Graph([(0, 1), (1, 2), (2, 3), (3, 0), (0, 2)])
    for g, want in ((nx.path_graph(4), 12), (nx.cycle_graph(4), 3), (nx.star_graph(3), 4), (paw, 12), (diamond, 6),
                    (nx.complete_graph(4), 1)):
        assert m4[_class_index(4, g), k4] == want, g.edges
    for g, want in ((nx.cycle_graph(5), 12), (nx.path_graph(5), 60), (nx.star_graph(4), 5)):
        assert m5[_class_index(5, g), k5] == want, g.edges
    assert m3[_class_index(3, nx.path_graph(3)), k3] == 3


@pytest.mark.parametrize("k", [2, 3, 4, 5, 6])
def test_transform_diagonal_and_edge_counts(k):
    classes = census_classes(k)
    assert len(classes) == {2: 1, 3: 2, 4: 6, 5: 21, 6: 112}[k]
    m = noninduced_matrix(k)
    assert m.dtype == np.int64 and m.shape == (len(classes), len(classes)) and (m >= 0).all()
    assert (np.diag(m) == 1).all()
    edges = np.array([len(e) for _, e in classes])
    assert (m[edges[:, None] > edges[None, :]] == 0).all()                  # c has fewer edges than q
    same = (edges[:, None] == edges[None, :]) & ~np.eye(len(classes), dtype=bool)
    assert (m[same] == 0).all()                                             # as many edges, another class
    assert (m[:, int(np.argmax(edges))] > 0).all()                          # everything occurs in K_k
    assert noninduced_matrix(k) is not m and (noninduced_matrix(k) == m).all()


def test_closed_form_on_complete_graphs():
    for n, queries in ((12, M.standard_nx()), (10, list(M.seven_node_queries().values()))):
        gs = GraphSet.from_edge_lists([(n, [(a, b) for a in range(n) for b in range(a + 1, n)])])
        want = np.array([M.complete_graph_counts(n, q) for q in queries]).T
        assert want[-1].min() >= 1 and want.max() > 10000
        for kw in (dict(), dict(method="matcher")):
            got = canonical_counts(gs, queries, backend="host", induced=False, **kw)
            assert got.long().tolist() == want.tolist(), kw


def test_stars():
    d = 41
    hub_last = GraphSet.from_edge_lists([(d + 1, [(i, d) for i in range(d)])])
    hub_first = GraphSet.from_edge_lists([(d + 1, [(0, i) for i in range(1, d + 1)])])
    k13, k12 = nx.star_graph(3), nx.star_graph(2)
    for kw in (dict(), dict(method="matcher")):
        got = canonical_counts(hub_last, [k13], backend="host", induced=False, **kw).reshape(-1).long().tolist()
        assert got == [0] * d + [math.comb(d, 3)], kw
        got = canonical_counts(hub_first, [k12], backend="host", induced=False, **kw).reshape(-1).long().tolist()
        assert got == [0] + [v - 1 for v in range(1, d + 1)], kw            # the leaves below leaf v
    # a star has no triangle: induced and non-induced stars coincide there
    assert torch.equal(canonical_counts(hub_last, [k13, k12], backend="host", induced=False),
                       canonical_counts(hub_last, [k13, k12], backend="host"))


@pytest.fixture(scope="module")
def census_inputs():
    graphs = golden_graphs(max_n=40) + random_family_graphs(3, 22)
    queries = M.standard_nx() + M.twelve_six_node_queries()
    gs = GraphSet.from_edge_lists(graphs)
    return gs, queries, canonical_counts(gs, queries, backend="host", induced=False, method="matcher")


def test_census_route_equals_matcher_route(census_inputs):
    gs, queries, matcher = census_inputs
    assert len(queries) == 41 and gs.num_graphs > 30
    census = canonical_counts(gs, queries, backend="host", induced=False)
    assert census.dtype == torch.double and (matcher.sum(0) > 0).all() and matcher.sum() > 1e6
    assert torch.equal(census, matcher)
    # duplicates and any query order are fine on the census route (classes are distinct by construction)
    mixed = [queries[40], queries[3], queries[3], queries[30], queries[0]]
    assert torch.equal(canonical_counts(gs, mixed, backend="host", induced=False), matcher[:, [40, 3, 3, 30, 0]])


def test_noninduced_bounds_induced(census_inputs):
    gs, queries, non = census_inputs
    ind = canonical_counts(gs, queries, backend="host")
    assert (non >= ind).all() and (non > ind).any()
    complete = [i for i, q in enumerate(queries) if q.number_of_edges() == len(q) * (len(q) - 1) // 2]
    assert [len(queries[i]) for i in complete] == [3, 4, 5, 6]
    assert torch.equal(non[:, complete], ind[:, complete]) and non[:, complete].sum() > 0


def test_labelled_matcher_equals_vf2_monomorphisms():
    graphs, labels, queries, want = M.labelled_yardstick(2)
    assert len(queries) == 100 and (want.sum(axis=0) > 0).sum() >= 60 and want[:, 84:].sum() > 0
    gs = GraphSet.from_edge_lists(graphs, node_feat=LV.features(labels, 2))
    got = canonical_counts_match_labelled(gs, queries, backend="host", induced=False)
    assert got.dtype == torch.double and got.long().tolist() == want.tolist()
    assert groundtruth.last_labelled_match_backend == "host"
    # the public entry sends every size to the labelled matcher (there is no labelled census)
    assert canonical_counts_labelled(gs, queries, backend="host", induced=False).long().tolist() == want.tolist()
    assert groundtruth.last_labelled_backend == "host"
    assert canonical_counts_labelled(gs, queries[:12], backend="vf2", induced=False).long().tolist() == \
        want[:, :12].tolist()
    # the default is still the induced count
    ind = canonical_counts_labelled(gs, queries, backend="host")
    assert torch.equal(ind, canonical_counts_labelled(gs, queries, backend="host", induced=True))
    assert (torch.from_numpy(want) >= ind.long()).all() and (torch.from_numpy(want) > ind.long()).any()


def test_unlabelled_equals_all_equal_labels():
    graphs = V.sparse_set()[:4] + V.dense_set()[:1]
    plain = [nx.path_graph(3), nx.cycle_graph(4), nx.star_graph(3), nx.path_graph(7), V.triangle_bridge_ring()]
    gs = GraphSet.from_edge_lists(graphs, node_feat=[np.ones((n, 1), np.float32) for n, _ in graphs])
    lab = [LV.labelled(q, {v: 0 for v in q}, 1) for q in plain]
    want = canonical_counts(gs, plain, backend="host", induced=False)
    assert (want.sum(0) > 0).all()
    assert torch.equal(canonical_counts_labelled(gs, lab, backend="host", induced=False), want)


def test_defaults_are_unchanged(census_inputs):
    queries = census_inputs[1]
    gs = GraphSet.from_edge_lists(V.sparse_set()[:4] + V.dense_set()[:1])
    seven = list(M.seven_node_queries().values())
    assert torch.equal(canonical_counts(gs, queries + seven, backend="host"),
                       canonical_counts(gs, queries + seven, backend="host", induced=True, method="auto"))
    assert torch.equal(canonical_counts_match(gs, seven, backend="host"),
                       canonical_counts_match(gs, seven, backend="host", induced=True))
    # method="matcher" with the default mode: the induced matcher at every size, equal to ESU
    assert torch.equal(canonical_counts(gs, queries, backend="host", method="matcher"),
                       canonical_counts(gs, queries, backend="host"))
    # the plan does not know the mode: one set of bytes, and computing non-induced counts leaves it alone
    before = match_plan(queries + seven).tobytes()
    canonical_counts(gs, seven, backend="host", induced=False)
    assert match_plan(queries + seven).tobytes() == before
    lq = M.labelled_queries()[:20]
    lbefore = [a.tobytes() for a in match_plan_labelled(lq)]
    graphs, labels, _ = M.labelled_inputs()
    lgs = GraphSet.from_edge_lists(graphs, node_feat=LV.features(labels, 2))
    canonical_counts_match_labelled(lgs, lq, backend="host", induced=False)
    assert [a.tobytes() for a in match_plan_labelled(lq)] == lbefore
    # induced = 1 through the new C entry is the old entry
    L = _lib.lib()
    plan = match_plan(seven)
    outs = [np.zeros((gs.num_nodes, len(seven)), np.int64) for _ in range(3)]
    head = (gs.graph_ptr.ctypes.data, gs.num_graphs, gs.rowptr.ctypes.data, gs.col.ctypes.data, plan.ctypes.data,
            len(plan), len(seven))
    assert L.desco_canonical_counts_match(*head, 1, outs[0].ctypes.data) == 0
    assert L.desco_canonical_counts_match_mode(*head, 1, 1, outs[1].ctypes.data) == 0
    assert L.desco_canonical_counts_match_mode(*head, 0, 1, outs[2].ctypes.data) == 0
    assert outs[0].sum() > 0 and (outs[0] == outs[1]).all() and (outs[2] >= outs[0]).all() and (outs[2] > outs[0]).any()


def test_workload_caches_the_two_truths_apart(tmp_path):
    from desco_amd.workload import Workload
    graphs = TRIANGLE + V.dense_set()[:1]
    queries = [nx.path_graph(3), nx.cycle_graph(4), nx.path_graph(7)]
    want = M.mono_counts(graphs, queries)
    w = Workload(GraphSet.from_edge_lists(graphs), str(tmp_path))
    assert not w.exist_groundtruth(None, queries) and not w.exist_groundtruth(None, queries, induced=False)
    t = w.compute_groundtruth(queries=queries, induced=False)
    assert t.dtype == torch.double and t.long().tolist() == want.tolist() and t[2, 0] == 3
    folder = tmp_path / "CanonicalCountTruth"
    assert (folder / "query_num_3_query_len_sum_14_noninduced.pt").exists()
    assert not (folder / "query_num_3_query_len_sum_14.pt").exists()
    assert w.exist_groundtruth(None, queries, induced=False) and not w.exist_groundtruth(None, queries)
    ind = w.compute_groundtruth(queries=queries)
    assert (folder / "query_num_3_query_len_sum_14.pt").exists() and ind[2, 0] == 0
    w2 = Workload(GraphSet.from_edge_lists(graphs), str(tmp_path))
    assert torch.equal(w2.load_groundtruth(None, queries, induced=False), t)
    assert torch.equal(w2.load_groundtruth(None, queries), ind) and not torch.equal(t, ind)
    # per-graph sums need no change: P3 in the triangle, 3 per graph
    assert w2.canonical_to_graphlet_truth(t)[0, 0] == 3


class _Reached(Exception):
    pass


@pytest.mark.parametrize("flag, induced", [([], True), (["--noninduced"], False)])
def test_main_passes_the_flag_to_compute_groundtruth(tmp_path, monkeypatch, flag, induced):
    import main as driver
    from desco_amd.workload import Workload
    seen = []

    def spy(self, query_ids=None, queries=None, num_workers=-1, save_to_file=True, induced=True):
        seen.append(induced)
        raise _Reached()

    monkeypatch.setattr(Workload, "compute_groundtruth", spy)
    monkeypatch.setattr(driver, "load_data", lambda name, root_folder=None: GraphSet.from_edge_lists(TRIANGLE))
    args, an, ag, ao = driver.parse_args(["--test_dataset", "TOY", "--test_gossip"] + flag)
    assert args.noninduced is (not induced) and ao.noninduced is (not induced) and ao.precision == "fp32"
    with pytest.raises(_Reached):
        driver.main(an, ag, ao, train_neighborhood=False, train_gossip=False, test_gossip=True,
                    neighborhood_checkpoint="none", gossip_checkpoint="none", atlas_query_ids=[6, 7],
                    output_dir=str(tmp_path / "out"), data_root=str(tmp_path))
    assert seen == [induced]


def test_refusals_name_the_limit():
    gs = GraphSet.from_edge_lists([(6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)])])
    p3, p7 = nx.path_graph(3), nx.path_graph(7)
    with pytest.raises(ValueError, match="unknown backend"):
        canonical_counts(gs, [p3], backend="cuda", induced=False)
    with pytest.raises(ValueError, match="unknown backend"):
        canonical_counts_match(gs, [p7], backend="vf2", induced=False)
    with pytest.raises(ValueError, match="unknown backend"):
        canonical_counts_labelled(gs, [], backend="esu", induced=False)
    for induced in (True, False):
        with pytest.raises(ValueError, match="unknown method"):
            canonical_counts(gs, [p3], backend="host", induced=induced, method="census")
    two_parts = nx.disjoint_union(nx.path_graph(2), nx.path_graph(2))
    for bad in (nx.path_graph(17), nx.path_graph(1), two_parts):
        for kw in (dict(), dict(method="matcher")):
            with pytest.raises(RuntimeError, match=r"connected and loop-free with 2\.\.16 nodes"):
                canonical_counts(gs, [p3, bad], backend="host", induced=False, **kw)
    assert canonical_counts(gs, [nx.path_graph(17)], backend="vf2", induced=False).sum() == 0     # the way out
    lgs = GraphSet.from_edge_lists([(6, [(0, 1), (1, 2)])], node_feat=[np.ones((6, 1), np.float32)])
    big = LV.labelled(nx.path_graph(17), {v: 0 for v in range(17)}, 1)
    with pytest.raises(RuntimeError, match=r"labelled queries of 2\.\.16 nodes"):
        canonical_counts_labelled(lgs, [big], backend="host", induced=False)
    assert canonical_counts_labelled(lgs, [big], backend="auto", induced=False).sum() == 0
    assert groundtruth.last_labelled_backend == "vf2"
    # the C entries: null arguments, a mode that is neither 0 nor 1, a plan of another size -- EINVAL with the name
    L = _lib.lib()
    plan = match_plan([p7])
    out = np.zeros((6, 1), np.int64)
    good = (gs.graph_ptr.ctypes.data, 1, gs.rowptr.ctypes.data, gs.col.ctypes.data, plan.ctypes.data, len(plan), 1)
    name = b"desco_canonical_counts_match_mode"
    for args in ((None,) + good[1:] + (0, 1, out.ctypes.data), good + (0, 1, None), good + (2, 1, out.ctypes.data),
                 good + (-1, 1, out.ctypes.data), good[:5] + (len(plan) - 1, 1, 0, 1, out.ctypes.data)):
        L.desco_rng_next(None, None, None)                                   # (another entry's message in between)
        assert L.desco_canonical_counts_match_mode(*args) == -1
        assert name in L.desco_last_error() and b"labelled" not in L.desco_last_error()
    assert L.desco_canonical_counts_match_mode(*good, 0, 1, out.ctypes.data) == 0 and out.sum() == 0
    lplan, _ = match_plan_labelled([LV.labelled(p7, {v: 0 for v in range(7)}, 1)])
    labels = np.zeros(6, np.int32)
    lgood = good[:4] + (labels.ctypes.data, lplan.ctypes.data, len(lplan), 1)
    name = b"desco_canonical_counts_match_labelled_mode"
    for args in (lgood + (0, 1, None), lgood[:4] + (None,) + lgood[5:] + (0, 1, out.ctypes.data),
                 lgood + (7, 1, out.ctypes.data), lgood[:6] + (len(lplan) + 1, 1, 0, 1, out.ctypes.data)):
        L.desco_rng_next(None, None, None)
        assert L.desco_canonical_counts_match_labelled_mode(*args) == -1
        assert name in L.desco_last_error()
    assert L.desco_canonical_counts_match_labelled_mode(*lgood, 0, 1, out.ctypes.data) == 0
    # the device entries validate on the host, before any HIP call
    for fn, nm in ((L.desco_canonical_counts_match_mode_dev, b"desco_canonical_counts_match_mode_dev"),
                   (L.desco_canonical_counts_match_labelled_mode_dev,
                    b"desco_canonical_counts_match_labelled_mode_dev")):
        n_args = len(_lib.SIGNATURES[nm.decode()][1])
        args = [None] * n_args
        ints = [i for i, t in enumerate(_lib.SIGNATURES[nm.decode()][1]) if t is not _lib.vp]
        for i in ints:
            args[i] = 1
        L.desco_rng_next(None, None, None)
        assert fn(*args) == -1 and nm in L.desco_last_error()
    L.desco_rng_next(None, None, None)
    assert L.desco_canonical_noninduced_transform_dev(None, 4, None, 5, 4, 3, 0, None, 3, None) == -1
    assert b"desco_canonical_noninduced_transform_dev" in L.desco_last_error()
    buf = np.zeros(64, np.int64).ctypes.data                                 # (never dereferenced: refused before)
    for c, q, ldc, ldo, acc in ((0, 3, 4, 3, 0), (33, 3, 33, 3, 0), (4, 65, 4, 65, 0), (4, 3, 3, 3, 0), (4, 3, 4, 2, 0),
                                (4, 3, 4, 3, 2)):
        assert L.desco_canonical_noninduced_transform_dev(buf, ldc, buf, 5, c, q, acc, buf, ldo, None) == -1
    assert L.desco_canonical_noninduced_transform_dev(None, 4, None, 0, 4, 3, 0, None, 3, None) == 0   # nothing to do
