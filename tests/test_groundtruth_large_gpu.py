"""Exact ground truth for queries of 7..16 nodes on the MI355X: the device matcher (csrc/groundtruth_match_dev.hip)
against the host matcher and networkx VF2 run as the reference runs it (groundtruth_vf2.py).  Integers, bit-exact.
Every case is sized so that VF2 or the host matcher finishes it in seconds."""
import networkx as nx
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import groundtruth_vf2 as V  # noqa: E402
from desco_amd import groundtruth, synthetic  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402
from desco_amd.groundtruth import (canonical_counts, canonical_counts_match,  # noqa: E402
                                   canonical_counts_match_device)


def hub_graph(seed=5, n=300, hubs=4, spokes=32):
    """A random tree on 300 nodes plus four hubs of about 32 spokes each."""
    rng = np.random.default_rng(seed)
    edges = {(int(rng.integers(0, i)), i) for i in range(1, n)}
    for h in rng.choice(n, hubs, replace=False):
        for u in rng.choice(n, spokes, replace=False):
            if u != h:
                edges.add((int(min(h, u)), int(max(h, u))))
    return n, sorted(edges)


@pytest.mark.parametrize("which", ["sparse", "dense"])
def test_device_equals_host_equals_vf2(which):
    graphs, names, queries, want = V.yardstick(which)
    V.check_nonzero([V.yardstick("sparse")[3], V.yardstick("dense")[3]], queries)
    gs = GraphSet.from_edge_lists(graphs)
    dev = canonical_counts_match_device(gs, queries)
    assert dev.dtype == torch.int64 and dev.is_cuda
    assert dev.cpu().tolist() == want.tolist()
    assert canonical_counts_match(gs, queries, backend="host").long().tolist() == want.tolist()
    # the public entry on this box: large columns to the device matcher, C6 to the ESU path
    assert canonical_counts(gs, queries).long().tolist() == want.tolist()


def test_device_equals_host_on_a_hub_graph():
    gs = GraphSet.from_edge_lists([hub_graph()])
    assert np.diff(gs.rowptr).max() >= 30
    queries = [nx.path_graph(7), nx.star_graph(6), nx.balanced_tree(2, 2)]
    host = canonical_counts_match(gs, queries, backend="host", num_threads=16).long()
    dev = canonical_counts_match_device(gs, queries).cpu()
    assert (host.sum(0) > 10000).all()
    assert dev.tolist() == host.tolist()


def test_device_equals_host_on_cox2():
    gs = synthetic.WORKLOADS["cox2"]()
    queries = [nx.path_graph(7), nx.cycle_graph(8), V.fused_rings()]
    host = canonical_counts_match(gs, queries, backend="host", num_threads=16).long()
    dev = canonical_counts_match_device(gs, queries).cpu()
    assert (host.sum(0) > 0).all()
    assert dev.tolist() == host.tolist()


def test_bitset_word_boundaries():
    """Graphs of 1, 2, 63, 64, 65 and 129 nodes: rows of one, two and three 64-bit words, in one set."""
    rng = np.random.default_rng(9)
    graphs = []
    for n in (1, 2, 63, 64, 65, 129):
        edges = {(int(rng.integers(0, i)), i) for i in range(1, n)}
        edges |= {(a, b) for a in range(n) for b in range(a + 1, n) if rng.random() < 2.0 / max(n, 1)}
        if n > 2:
            edges |= {(0, n - 1), (n - 2, n - 1), (min(62, n - 3), n - 1)}        # the last bit of the last word is used
        graphs.append((n, sorted(edges)))
    gs = GraphSet.from_edge_lists(graphs)
    queries = [nx.path_graph(7), nx.cycle_graph(7), nx.balanced_tree(2, 2), nx.path_graph(2), nx.path_graph(3),
               V.triangle_bridge_ring()]
    host = canonical_counts_match(gs, queries, backend="host").long()
    dev = canonical_counts_match_device(gs, queries).cpu()
    assert host[-129:].sum() > 1000 and host[:3].sum() == 1 and (host.sum(0) > 0).all()
    assert dev.tolist() == host.tolist()


def test_two_launches_are_bit_identical_and_slicing_does_not_change_the_result():
    graphs = V.dense_set() + V.sparse_set()[:4]
    gs = GraphSet.from_edge_lists(graphs)
    queries = list(V.large_queries().values())[:5]
    one = canonical_counts_match_device(gs, queries, slice_entries=int(gs.col.shape[0]))
    again = canonical_counts_match_device(gs, queries, slice_entries=int(gs.col.shape[0]))
    assert one.sum() > 1000 and torch.equal(one, again)
    for slice_entries in (150, 97, 7):
        assert int(gs.col.shape[0]) > 3 * slice_entries
        cut = canonical_counts_match_device(gs, queries, slice_entries=slice_entries)
        assert torch.equal(cut, one), slice_entries
    assert torch.equal(canonical_counts_match(gs, queries, backend="device", slice_entries=50).long(), one.cpu())
    assert one.cpu().tolist() == canonical_counts_match(gs, queries, backend="host").long().tolist()


def test_auto_picks_the_device_and_the_host_above_the_bitset_limit(monkeypatch):
    gs = GraphSet.from_edge_lists(V.dense_set())
    queries = [nx.path_graph(7), nx.cycle_graph(8)]
    host = canonical_counts_match(gs, queries, backend="host")
    assert groundtruth.last_match_backend == "host"
    assert torch.equal(canonical_counts_match(gs, queries, backend="auto"), host)
    assert groundtruth.last_match_backend == "device"
    monkeypatch.setattr(groundtruth, "_DEVICE_BITSET_LIMIT_WORDS", 10)
    assert torch.equal(canonical_counts_match(gs, queries, backend="auto"), host)
    assert groundtruth.last_match_backend == "host"
    assert torch.equal(canonical_counts(gs, queries), host)                      # routed the same way
    assert groundtruth.last_match_backend == "host"


def test_degenerate_sets_and_refusals_on_the_device():
    queries = [nx.path_graph(7), nx.star_graph(6)]
    for graphs in ([(1, [])], [(9, [])], [(1, []), (2, [(0, 1)])]):
        got = canonical_counts_match_device(GraphSet.from_edge_lists(graphs), queries)
        assert got.shape == (sum(n for n, _ in graphs), 2) and got.sum() == 0
    gs = GraphSet.from_edge_lists([(6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)])])
    with pytest.raises(RuntimeError, match=r"2\.\.16 nodes"):
        canonical_counts_match_device(gs, [nx.path_graph(17)])
    assert canonical_counts_match_device(gs, [nx.path_graph(6), nx.path_graph(2)]).sum(0).tolist() == [1, 5]
