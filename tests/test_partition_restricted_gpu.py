"""Device builder in restricted mode (build_partition_device(restricted=True), csrc/partition_dev.hip) against the host
builder in the same mode: integer work, every array bit for bit."""
import numpy as np
import pytest

from helpers import golden_graphs

pytestmark = pytest.mark.gpu

from desco_amd.graphs import GraphSet
from desco_amd.partition import build_partition, build_partition_device

FIELDS = ("neigh_index", "indicator", "count_ptr", "count_orig", "vrowptr", "vcol")
FIVE_CYCLE = (6, [(3, 5), (5, 0), (0, 1), (1, 2), (2, 3)])


def _same(a, b):
    assert a.restricted and b.restricted
    assert (a.num_neigh, a.num_count, a.num_edges) == (b.num_neigh, b.num_count, b.num_edges)
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape, (f, x.shape, y.shape)
        assert np.array_equal(x, y), f


def test_five_cycle():
    gs = GraphSet.from_edge_lists([FIVE_CYCLE])
    dev = build_partition_device(gs, 2, restricted=True)
    _same(dev, build_partition(gs, 2, restricted=True))
    b = dev.neigh_index.tolist().index([0, 3])
    assert dev.count_orig[dev.count_ptr[b]:dev.count_ptr[b + 1]].tolist() == [1, 2]
    ball = build_partition_device(gs, 2)                          # the other definition reaches 0 through 5
    assert ball.count_orig[ball.count_ptr[b]:ball.count_ptr[b + 1]].tolist() == [0, 1, 2]


@pytest.mark.parametrize("depth", [0, 1, 2, 4])
def test_golden_graphs_bit_exact(depth):
    gs = GraphSet.from_edge_lists(golden_graphs())
    _same(build_partition_device(gs, depth, restricted=True), build_partition(gs, depth, restricted=True))


def test_edgeless_graph_isolated_nodes_and_a_hub():
    graphs = [(3, []), (2, [(0, 1)]), (7, [(1, 2), (2, 5)]), (3, [(0, 1), (1, 2), (0, 2)]),
              (72, [(71, i) for i in range(71)]), (72, [(0, i) for i in range(1, 72)]), (1, [])]
    gs = GraphSet.from_edge_lists(graphs)
    _same(build_partition_device(gs, 4, restricted=True), build_partition(gs, 4, restricted=True))
    empty = build_partition_device(GraphSet.from_edge_lists([(2, [])]), 4, restricted=True)
    assert empty.num_neigh == 0 and empty.num_edges == 0 and not empty.indicator.any()


def test_large_graph_multiword_bitmaps_depth_3():
    rng = np.random.default_rng(5)

    def tree_plus(n, extra):
        edges = [(i, int(rng.integers(0, i))) for i in range(1, n)]
        edges += [(int(a), int(b)) for a, b in rng.integers(0, n, size=(extra, 2)) if a != b]
        return (n, edges)
    mid = GraphSet.from_edge_lists([tree_plus(3000, 1500)])
    dev, host = build_partition_device(mid, 3, restricted=True), build_partition(mid, 3, restricted=True)
    _same(dev, host)
    assert np.diff(host.count_ptr).max() > 32                    # neighborhoods that span several bitmap words


def test_few_waves_and_many_waves_agree():
    gs = GraphSet.from_edge_lists(golden_graphs(max_n=60) + [FIVE_CYCLE])
    host = build_partition(gs, 4, restricted=True)
    _same(build_partition_device(gs, 4, num_waves=4, restricted=True), host)
    _same(build_partition_device(gs, 4, num_waves=4096, restricted=True), host)


def test_device_slices_and_degree_sort_keep_the_mode():
    gs = GraphSet.from_edge_lists(golden_graphs(max_n=30))
    dev, host = build_partition_device(gs, 3, restricted=True), build_partition(gs, 3, restricted=True)
    _same(dev.slice_device(2, 9), host.slice(2, 9))
    _same(dev.degree_sorted_device(), host.degree_sorted())
