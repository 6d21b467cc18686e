"""Host builder in restricted mode (build_partition(restricted=True): the homogeneous ablation's neighborhoods) against a
Python restatement of the reference's k_neigh_canonical plus the edge rule, and against the node sets the reference's own
get_neigh_canonical produced (tests/golden/partition_homo_golden.json).  Integer work: everything is compared exactly."""
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN, golden_graphs, random_family_graphs

from desco_amd import _lib
from desco_amd.graphs import GraphSet
from desco_amd.partition import SLOT_EDGE_TYPES_CANON_DST, SLOT_EDGE_TYPES_COUNT_DST, build_partition

# the 5-cycle 3-5-0-1-2-3: node 0 is two steps from node 3 only through node 5
FIVE_CYCLE = (6, [(3, 5), (5, 0), (0, 1), (1, 2), (2, 3)])


def adjacency(n, edges):
    adj = [set() for _ in range(n)]
    for a, b in edges:
        adj[a].add(b)
        adj[b].add(a)
    return adj


def restricted_nodes(adj, v, depth):
    """k_neigh_canonical: `depth` rounds, a neighbour w is taken iff w <= v and it is not yet marked."""
    seen, front = {v}, {v}
    for _ in range(depth):
        front = {w for u in front for w in adj[u] if w <= v} - seen
        seen |= front
    return seen


def expected_partition(graphs, depth):
    """Per kept neighborhood (ascending graph, node): (graph id, v, sorted nodes, {(src, dst): (edge type)}); and the
    indicator of every node."""
    neighs, indicator = [], []
    for gid, (n, edges) in enumerate(graphs):
        adj = adjacency(n, edges)
        for v in range(n):
            nodes = restricted_nodes(adj, v, depth)
            typed = {}
            for a in nodes:
                for b in adj[a] & nodes:                               # directed edge b -> a
                    tri = bool(adj[a] & adj[b] & nodes)
                    typed[(b, a)] = ("canonical" if b == v else "count",
                                     "union_triangle" if tri else "union_tride",
                                     "canonical" if a == v else "count")
            indicator.append(bool(typed))
            if typed:                                                  # a neighborhood without an edge is skipped
                neighs.append((gid, v, sorted(nodes), typed))
    return neighs, indicator


def check_against_restatement(graphs, depth):
    part = build_partition(GraphSet.from_edge_lists(graphs), depth, restricted=True)
    assert part.restricted and part.depth == depth
    want, indicator = expected_partition(graphs, depth)
    assert part.indicator.tolist() == indicator
    assert part.neigh_index.tolist() == [[g, v] for g, v, _, _ in want]
    gptr = np.concatenate([[0], np.cumsum([n for n, _ in graphs])])
    Nc, B = part.num_count, part.num_neigh
    owner = np.concatenate([np.repeat(np.arange(B), np.diff(part.count_ptr)), np.arange(B)]).astype(np.int64)
    orig = np.concatenate([part.count_orig - gptr[part.neigh_index[owner[:Nc], 0]], part.neigh_index[:, 1]])
    got = [dict() for _ in range(B)]
    eid = part.edge_index_dict()
    assert set(eid) == set(SLOT_EDGE_TYPES_COUNT_DST) | set(SLOT_EDGE_TYPES_CANON_DST)
    for (s, rel, d), ei in eid.items():
        src = ei[0] + (Nc if s == "canonical" else 0)
        dst = ei[1] + (Nc if d == "canonical" else 0)
        assert (owner[src] == owner[dst]).all()
        for b, a_, b_ in zip(owner[src].tolist(), orig[src].tolist(), orig[dst].tolist()):
            assert (a_, b_) not in got[b]
            got[b][(a_, b_)] = (s, rel, d)
    for b, (gid, v, nodes, typed) in enumerate(want):
        c0, c1 = part.count_ptr[b], part.count_ptr[b + 1]
        assert (part.count_orig[c0:c1] - gptr[gid]).tolist() + [v] == nodes, (gid, v)    # ascending, canonical last
        assert got[b] == typed, (gid, v)
    # sources ascending inside every slot
    for r in range(4 * (Nc + B)):
        seg = part.vcol[part.vrowptr[r]:part.vrowptr[r + 1]]
        assert (np.diff(seg) > 0).all()
    return part


def neighborhood_nodes(part, graphs, gid, v):
    b = part.neigh_index.tolist().index([gid, v])
    base = int(np.cumsum([0] + [n for n, _ in graphs])[gid])
    return set((part.count_orig[part.count_ptr[b]:part.count_ptr[b + 1]] - base).tolist()) | {v}


def test_five_cycle_separates_the_two_definitions():
    graphs = [FIVE_CYCLE]
    gs = GraphSet.from_edge_lists(graphs)
    restricted = check_against_restatement(graphs, 2)
    assert neighborhood_nodes(restricted, graphs, 0, 3) == {1, 2, 3}
    ball = build_partition(gs, 2)
    assert not ball.restricted
    assert neighborhood_nodes(ball, graphs, 0, 3) == {0, 1, 2, 3}


@pytest.mark.parametrize("depth", [0, 1, 2, 4])
def test_golden_graphs_against_restatement(depth):
    check_against_restatement(golden_graphs(), depth)


@pytest.mark.parametrize("seed,depth", [(41, 1), (42, 2), (43, 4)])
def test_random_families_with_shuffled_ids(seed, depth):
    check_against_restatement(random_family_graphs(seed, 44), depth)


@pytest.mark.parametrize("depth", [0, 1, 4])
def test_isolated_nodes_and_edgeless_graphs(depth):
    graphs = [(3, []), (2, [(0, 1)]), (7, [(1, 2), (2, 5)]), (1, []), (3, [(0, 1), (1, 2), (0, 2)])]
    part = check_against_restatement(graphs, depth)
    if depth == 0:
        assert part.num_neigh == 0 and part.num_edges == 0 and not part.indicator.any()
    else:
        assert part.indicator.tolist() == [False] * 3 + [False, True] + [False, False, True, False, False, True, False] + \
            [False] + [False, True, True]


def test_restricted_is_a_connected_subset_of_the_ball_definition():
    graphs = random_family_graphs(44, 33)
    gs = GraphSet.from_edge_lists(graphs)
    for depth in (1, 3):
        r, h = build_partition(gs, depth, restricted=True), build_partition(gs, depth)
        assert r.indicator.tolist() == h.indicator.tolist()          # v has a neighbour <= v in both or in neither
        for b, (gid, v) in enumerate(r.neigh_index.tolist()):
            assert neighborhood_nodes(r, graphs, gid, v) <= neighborhood_nodes(h, graphs, gid, v)


def test_reference_node_sets():
    """partition_homo_golden.json holds what the reference's own get_neigh_canonical returned (node set, edge count) for
    every node of the golden graphs and the 5-cycle at depths 0, 1, 2 and 4."""
    with open(os.path.join(GOLDEN, "partition_homo_golden.json")) as f:
        gold = json.load(f)
    graphs = [(g["n"], [tuple(e) for e in g["edges"]]) for g in gold["graphs"]]
    assert graphs[0] == (FIVE_CYCLE[0], list(FIVE_CYCLE[1]))
    assert gold["graphs"][0]["neighs"]["2"]["nodes"][3] == [1, 2, 3]
    gs = GraphSet.from_edge_lists(graphs)
    gptr = np.concatenate([[0], np.cumsum([n for n, _ in graphs])])
    assert gold["depths"] == [0, 1, 2, 4]
    for depth in gold["depths"]:
        part = build_partition(gs, depth, restricted=True)
        deg = np.diff(part.vrowptr.astype(np.int64)).reshape(-1, 4).sum(1)
        b = 0
        for gid, g in enumerate(gold["graphs"]):
            ref = g["neighs"][str(depth)]
            for v in range(g["n"]):
                kept = ref["num_edges"][v] > 0
                assert bool(part.indicator[gptr[gid] + v]) == kept
                if not kept:
                    continue
                assert part.neigh_index[b].tolist() == [gid, v]
                c0, c1 = part.count_ptr[b], part.count_ptr[b + 1]
                assert (part.count_orig[c0:c1] - gptr[gid]).tolist() + [v] == ref["nodes"][v]
                assert deg[c0:c1].sum() + deg[part.num_count + b] == 2 * ref["num_edges"][v]   # both directions
                b += 1
        assert b == part.num_neigh


def test_quirk_emulation_is_refused_in_restricted_mode():
    gs = GraphSet.from_edge_lists([FIVE_CYCLE])
    with pytest.raises(ValueError, match="quirk_batch is not offered with restricted=True"):
        build_partition(gs, 2, quirk_batch=4, restricted=True)
    import ctypes
    L, handle = _lib.lib(), ctypes.c_void_p()
    rc = L.desco_partition_build_mode(gs.graph_ptr.ctypes.data, gs.num_graphs, gs.rowptr.ctypes.data, gs.col.ctypes.data,
                                      2, 1, 4, 1, ctypes.byref(handle))
    assert rc == -1 and b"quirk_batch" in L.desco_last_error() and not handle.value
    rc = L.desco_partition_build_mode(gs.graph_ptr.ctypes.data, gs.num_graphs, gs.rowptr.ctypes.data, gs.col.ctypes.data,
                                      2, 7, 0, 1, ctypes.byref(handle))
    assert rc == -1 and b"unknown neighborhood mode" in L.desco_last_error()
    # device entry points refuse an unknown mode on the host, before any HIP call
    assert L.desco_partition_dev_count_mode(None, None, None, None, 4, 2, 7, 8, 4, None, None, None, None) == -1
    assert b"desco_partition_dev_count_mode" in L.desco_last_error()
    assert L.desco_partition_dev_fill_mode(None, None, None, None, 4, 2, 7, 8, 4, *([None] * 4), 0, 0, 0, 0,
                                           *([None] * 6), None) == -1
    assert b"desco_partition_dev_fill_mode" in L.desco_last_error()


def test_slices_and_degree_sort_keep_the_mode():
    part = build_partition(GraphSet.from_edge_lists(golden_graphs(max_n=30)), 3, restricted=True)
    assert part.slice(2, 9).restricted and part.select([1, 4, 5]).restricted and part.degree_sorted().restricted
    assert "restricted=True" in repr(part)
