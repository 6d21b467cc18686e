"""Exact NON-INDUCED ground truth on the MI355X: the device matcher's non-induced instantiations and the device census +
transform kernel against the host routes (which tests/test_groundtruth_noninduced_host.py holds against VF2), bit for
bit.  Every graph has at most 60 nodes; a 41-leaf star, K12 and K10 stand for hubs and dense targets."""
import math

import networkx as nx
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import groundtruth_labelled_vf2 as LV  # noqa: E402
import groundtruth_mono_vf2 as M  # noqa: E402
import groundtruth_vf2 as V  # noqa: E402
from desco_amd import groundtruth  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402
from desco_amd.groundtruth import (canonical_counts, canonical_counts_device, canonical_counts_labelled,  # noqa: E402
                                   canonical_counts_match, canonical_counts_match_device,
                                   canonical_counts_match_labelled, canonical_counts_match_labelled_device,
                                   noninduced_transform_device)
from helpers import golden_graphs, random_family_graphs  # noqa: E402

D = 41


def complete(n):
    return n, [(a, b) for a in range(n) for b in range(a + 1, n)]


def small_graphs():
    """golden graphs and random families of at most 40 nodes (without the one G(35, 0.45) of 271 edges, whose 2e8
    seven-node occurrences would take the host five seconds), four sparse molecule-like graphs, a G(18, 0.3), the star
    with 41 leaves and its hub last, and K12"""
    families = [g for g in random_family_graphs(3, 22) if len(g[1]) <= 200]
    assert len(families) == 21
    return (golden_graphs(max_n=40)[:10] + families + V.sparse_set()[:4] + V.dense_set()[:1] +
            [(D + 1, [(i, D) for i in range(D)]), complete(12)])


@pytest.fixture(scope="module")
def unlabelled():
    graphs = small_graphs()
    assert max(n for n, _ in graphs) <= 60
    gs = GraphSet.from_edge_lists(graphs)
    queries = M.standard_nx() + M.twelve_six_node_queries() + list(M.seven_node_queries().values())
    host = canonical_counts_match(gs, queries, backend="host", induced=False).long()
    assert (host.sum(0) > 0).all() and host.sum() > 1e6
    return gs, queries, host


@pytest.fixture(scope="module")
def labelled():
    graphs, labels, _ = M.labelled_inputs(2)
    graphs = graphs + [complete(9)]
    labels = labels + [np.arange(9) % 2]
    gs = GraphSet.from_edge_lists(graphs, node_feat=LV.features(labels, 2))
    queries = M.labelled_queries(2)
    host = canonical_counts_match_labelled(gs, queries, backend="host", induced=False).long()
    assert (host.sum(0) > 0).sum() >= 90 and host[:, 84:].sum() > 0
    return gs, queries, host


def test_device_matcher_equals_host_matcher(unlabelled):
    gs, queries, host = unlabelled
    dev = canonical_counts_match_device(gs, queries, induced=False)
    assert dev.dtype == torch.int64 and dev.is_cuda
    assert dev.cpu().tolist() == host.tolist()
    assert canonical_counts_match(gs, queries, backend="device", induced=False).long().tolist() == host.tolist()
    assert groundtruth.last_match_backend == "device"
    induced = canonical_counts_match(gs, queries, backend="host").long()
    assert (host >= induced).all() and (host > induced).any()


def test_device_labelled_matcher_equals_host_matcher(labelled):
    gs, queries, host = labelled
    dev = canonical_counts_match_labelled_device(gs, queries, induced=False)
    assert dev.dtype == torch.int64 and dev.is_cuda and dev.cpu().tolist() == host.tolist()
    assert canonical_counts_match_labelled(gs, queries, backend="device", induced=False).long().tolist() == host.tolist()
    assert canonical_counts_labelled(gs, queries, induced=False).long().tolist() == host.tolist()
    assert groundtruth.last_labelled_backend == "device"


def test_slicing_and_repetition_do_not_change_the_result(unlabelled, labelled):
    """``slice_entries`` of 1, 7 and the default, and two runs.  Every slice is a launch and a synchronisation, so the
    one-entry slices run on the first four graphs only."""
    gs, queries, host = unlabelled
    sel = [0, 3, 10, 28, 29, 40, 41, 43, 45]                     # sizes 3..7
    qs = [queries[i] for i in sel]
    for count, slices in ((12, (7,)), (4, (1, 7))):
        sub = GraphSet.from_edge_lists(gs.edge_lists()[:count])
        one = canonical_counts_match_device(sub, qs, induced=False)
        assert one.sum() > 100 and one.cpu().tolist() == host[:sub.num_nodes][:, sel].tolist()
        assert torch.equal(canonical_counts_match_device(sub, qs, induced=False), one)
        for slice_entries in slices:
            assert int(sub.col.shape[0]) > 3 * slice_entries
            assert torch.equal(canonical_counts_match_device(sub, qs, slice_entries=slice_entries, induced=False), one)
    lgs, lqueries, lhost = labelled
    lsub = lgs.subset(0, 1)
    lone = canonical_counts_match_labelled_device(lsub, lqueries, induced=False)
    assert lone.sum() > 100 and lone.cpu().tolist() == lhost[:lsub.num_nodes].tolist()
    assert torch.equal(canonical_counts_match_labelled_device(lsub, lqueries, induced=False), lone)
    for slice_entries in (1, 7):
        assert int(lsub.col.shape[0]) > 3 * slice_entries
        assert torch.equal(canonical_counts_match_labelled_device(lsub, lqueries, slice_entries=slice_entries,
                                                                  induced=False), lone)


def test_device_census_and_transform_equal_host_and_matcher_routes(unlabelled):
    gs, queries, host = unlabelled
    std = queries[:29]
    dev = canonical_counts_device(gs, std, induced=False)
    assert dev.dtype == torch.int64 and dev.is_cuda and dev.shape == (gs.num_nodes, 29)
    assert dev.cpu().tolist() == host[:, :29].tolist()                               # the matcher route
    assert canonical_counts(gs, std, backend="host", induced=False).long().tolist() == dev.cpu().tolist()
    # duplicates, any order and a two-node query are fine: the census classes are distinct by construction
    mixed = [std[5], nx.path_graph(2), std[5], std[28], std[0]]
    got = canonical_counts_device(gs, mixed, induced=False).cpu()
    assert got[:, [0, 2, 3, 4]].tolist() == host[:, [5, 5, 28, 0]].tolist()
    assert got[:, 1].tolist() == [int((gs.col[gs.rowptr[v]:gs.rowptr[v + 1]] < v).sum()) for v in range(gs.num_nodes)]
    # the public entry: 3..5 nodes by the device census, 6 nodes by the host census, 7 nodes by the device matcher
    for backend in ("auto", "device"):
        cols = list(range(len(queries))) if backend == "auto" else list(range(29)) + list(range(41, 46))
        got = canonical_counts(gs, [queries[i] for i in cols], backend=backend, induced=False)
        assert got.dtype == torch.double and got.long().tolist() == host[:, cols].tolist(), backend
    with pytest.raises(RuntimeError, match=r"2\.\.5 nodes"):
        canonical_counts_device(gs, [queries[30]], induced=False)
    with pytest.raises(RuntimeError, match=r"2\.\.5 nodes"):
        canonical_counts(gs, [queries[30]], backend="device", induced=False)


def test_closed_forms_on_the_device():
    for n, queries in ((12, M.standard_nx()), (10, list(M.seven_node_queries().values()))):
        gs = GraphSet.from_edge_lists([complete(n)])
        want = np.array([M.complete_graph_counts(n, q) for q in queries]).T
        assert canonical_counts_match_device(gs, queries, induced=False).cpu().tolist() == want.tolist()
        if n == 12:
            assert canonical_counts_device(gs, queries, induced=False).cpu().tolist() == want.tolist()
    hub_last = GraphSet.from_edge_lists([(D + 1, [(i, D) for i in range(D)])])
    hub_first = GraphSet.from_edge_lists([(D + 1, [(0, i) for i in range(1, D + 1)])])
    for fn in (canonical_counts_device, canonical_counts_match_device):
        assert fn(hub_last, [nx.star_graph(3)], induced=False).reshape(-1).tolist() == [0] * D + [math.comb(D, 3)]
        assert fn(hub_first, [nx.star_graph(2)], induced=False).reshape(-1).tolist() == \
            [0] + [v - 1 for v in range(1, D + 1)]
    tri = GraphSet.from_edge_lists([complete(3)])
    assert canonical_counts_device(tri, [nx.path_graph(3)], induced=False).reshape(-1).tolist() == [0, 0, 3]
    assert canonical_counts_device(tri, [nx.path_graph(3)]).reshape(-1).tolist() == [0, 0, 0]


@pytest.mark.parametrize("n, c, q", [(1, 1, 1), (257, 32, 29), (300, 21, 1), (64, 1, 29), (1000, 30, 29), (5, 7, 3)])
def test_transform_kernel_equals_numpy_int64(n, c, q):
    rng = np.random.default_rng(1000 * n + 32 * c + q)
    census = rng.integers(0, 1 << 20, size=(n, c), dtype=np.int64)
    m = rng.integers(0, 1 << 12, size=(c, q), dtype=np.int64)
    census[rng.random((n, c)) < 0.1] = (1 << 53) + 1                 # beyond a double's integers
    census[0, 0] = (1 << 62) + 12345
    m[0, 0] = 1
    with np.errstate(over="ignore"):
        want = census @ m                                             # int64, modulo 2^64 like the kernel
    assert int(want.max()) > 1 << 53 or n * c == 1
    census_d = torch.from_numpy(census).cuda()
    got = noninduced_transform_device(census_d, m)
    assert got.dtype == torch.int64 and got.is_cuda and got.shape == (n, q)
    assert np.array_equal(got.cpu().numpy(), want)
    # adding a second chunk into the result, and reading a census that is a column slice of a wider tensor
    with np.errstate(over="ignore"):
        want2 = want + census[:, ::-1] @ m
    wide = torch.from_numpy(np.concatenate([census[:, ::-1], census], axis=1)).cuda()
    assert noninduced_transform_device(wide[:, :c].contiguous(), m, accumulate_into=got) is got
    assert np.array_equal(got.cpu().numpy(), want2)
    # exact where a double would not be: 2^53 + 1 survives
    one = torch.full((1, 1), (1 << 53) + 1, dtype=torch.int64, device="cuda")
    assert int(noninduced_transform_device(one, np.ones((1, 1), np.int64))[0, 0]) == (1 << 53) + 1


def test_induced_device_calls_are_unchanged(unlabelled, labelled):
    gs, queries, _ = unlabelled
    std, seven = queries[:29], queries[41:]
    esu = canonical_counts(gs, std, backend="host").long()
    assert esu.sum() > 1000
    assert canonical_counts_device(gs, std).cpu().tolist() == esu.tolist()
    assert torch.equal(canonical_counts_device(gs, std, induced=True), canonical_counts_device(gs, std))
    host7 = canonical_counts_match(gs, seven, backend="host").long()
    assert host7.sum() > 1000
    assert canonical_counts_match_device(gs, seven).cpu().tolist() == host7.tolist()
    assert torch.equal(canonical_counts_match_device(gs, seven, induced=True), canonical_counts_match_device(gs, seven))
    lgs, lqueries, lhost = labelled
    lind = canonical_counts_match_labelled(lgs, lqueries, backend="host").long()
    assert lind.sum() > 100 and not torch.equal(lind, lhost)
    assert canonical_counts_match_labelled_device(lgs, lqueries).cpu().tolist() == lind.tolist()
    assert torch.equal(canonical_counts_match_labelled_device(lgs, lqueries, induced=True),
                       canonical_counts_match_labelled_device(lgs, lqueries))
