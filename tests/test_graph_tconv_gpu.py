"""The device builder of ``GraphBatch``'s typed CSR (desco_graph_tconv_dev) against its host twin, bit for bit."""
import functools

import numpy as np
import pytest
import torch

from desco_amd import ops, synthetic
from desco_amd.batch import GraphBatch, _graphset_device_csr
from desco_amd.graphs import GraphSet
from helpers import random_family_graphs
from test_graph_tconv_host import CASES, check_invariants

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def clique(k):
    return k, [(a, b) for a in range(k) for b in range(a + 1, k)]


def rows_of_degree(deg):
    """A hub of degree ``deg`` whose spokes form a path (every hub edge is a triangle edge, the ends of the path have
    degree 2, its inner nodes 3) with a tail of tride edges at the path's end, next to a clique of deg + 1 nodes (every
    row has degree ``deg`` and every test walks two rows of that length)."""
    hub = (deg + 4, [(0, v) for v in range(1, deg + 1)] + [(v, v + 1) for v in range(1, deg)] +
           [(deg, deg + 1), (deg + 1, deg + 2), (deg + 2, deg + 3)])
    return [hub, clique(deg + 1)]


def star_with_chords(spokes=300, chords=40, seed=0):
    rng = np.random.default_rng(seed)
    e = {(0, v) for v in range(1, spokes + 1)}
    while len(e) < spokes + chords:
        a, b = (int(v) for v in rng.integers(1, spokes + 1, size=2))
        if a != b:
            e.add((min(a, b), max(a, b)))
    return [(spokes + 1, sorted(e))]


def tree_with_hubs(n=300, hubs=4, spokes=32, seed=1):
    """hubs * (spokes + 1) nodes are four stars; the rest hangs off random earlier nodes; labels shuffled"""
    rng = np.random.default_rng(seed)
    e, v = [], 0
    centres = []
    for _ in range(hubs):
        centres.append(v)
        e += [(v, v + 1 + s) for s in range(spokes)]
        v += spokes + 1
    e += [(centres[i], centres[i + 1]) for i in range(hubs - 1)]
    e += [(int(rng.integers(w)), w) for w in range(v, n)]
    perm = rng.permutation(n)
    return [(n, sorted((int(min(perm[a], perm[b])), int(max(perm[a], perm[b]))) for a, b in e))]


@functools.lru_cache(maxsize=None)
def big_set(name):
    """the Syn_1827- and COX2-shaped sets, generated once per session (the former takes seconds)"""
    if name == "syn_1827[300:420]":
        return big_set("syn_1827").subset(300, 420)
    return synthetic.WORKLOADS[name]()


def graph_set(name):
    if name in CASES:
        return GraphSet.from_edge_lists(CASES[name])
    if name.startswith("degree "):
        return GraphSet.from_edge_lists(rows_of_degree(int(name.split()[1])))
    if name == "star 300 + 40 chords":
        return GraphSet.from_edge_lists(star_with_chords())
    if name == "tree 300 with four 32-spoke hubs":
        return GraphSet.from_edge_lists(tree_with_hubs())
    return big_set(name)


NAMES = list(CASES) + ["degree 63", "degree 64", "degree 65", "degree 129", "star 300 + 40 chords",
                       "tree 300 with four 32-spoke hubs", "syn_1827[300:420]", "cox2"]


def device_arrays(gs, g0=0, g1=None):
    g1 = gs.num_graphs if g1 is None else g1
    n0, n1 = int(gs.graph_ptr[g0]), int(gs.graph_ptr[g1])
    e0, e1 = int(gs.rowptr[n0]), int(gs.rowptr[n1])
    rowptr, col = _graphset_device_csr(gs, DEV)
    return ops.graph_tconv_dev(rowptr, col, n0, n1 - n0, e0, e1 - e0)


@pytest.mark.parametrize("name", NAMES)
def test_device_builder_equals_the_host_twin(name):
    gs = graph_set(name)
    ref_ptr, ref_col = ops.graph_tconv_host(gs.rowptr, gs.col, 0, gs.num_nodes)
    if gs.num_nodes <= 2000:
        check_invariants(gs.edge_lists(), ref_ptr, ref_col)
    vrowptr, vcol = device_arrays(gs)
    again = device_arrays(gs)
    torch.cuda.synchronize()
    assert vrowptr.dtype == torch.int32 and vcol.dtype == torch.int32
    assert np.array_equal(vrowptr.cpu().numpy(), ref_ptr), name
    assert np.array_equal(vcol.cpu().numpy(), ref_col), name
    assert torch.equal(again[0], vrowptr) and torch.equal(again[1], vcol), "two launches differ"
    ntri = int((ref_ptr[1::2] - ref_ptr[:-1:2]).sum())
    print(f"[tconv] {name}: {gs.num_nodes} nodes, {len(gs.col)} directed edges, {ntri} triangle, largest degree "
          f"{int(np.diff(gs.rowptr).max()) if gs.num_nodes else 0}")


def test_hub_cases_have_the_rows_they_are_named_for():
    for deg in (63, 64, 65, 129):
        d = np.diff(graph_set(f"degree {deg}").rowptr)
        assert d.max() == deg and (d == deg).sum() >= deg + 1
    star = graph_set("star 300 + 40 chords")
    assert np.diff(star.rowptr).max() == 300 and len(star.col) == 2 * 340
    assert sorted(np.diff(graph_set("tree 300 with four 32-spoke hubs").rowptr))[-4] >= 32


@pytest.mark.parametrize("name", ["random families", "syn_1827[300:420]"])
def test_graph_batch_over_a_range_is_the_slice_of_the_whole_set(name):
    gs = graph_set(name)
    whole = GraphBatch(gs, DEV)
    assert whole.vrowptr.is_cuda and whole.vcol.is_cuda and whole.graph_ptr.is_cuda
    G = gs.num_graphs
    for g0, g1 in ((0, 1), (G // 3, 2 * G // 3), (G // 2, G // 2), (G - 5, G)):
        gb = GraphBatch(gs, DEV, g0, g1)
        n0, n1 = int(gs.graph_ptr[g0]), int(gs.graph_ptr[g1])
        e0, e1 = int(gs.rowptr[n0]), int(gs.rowptr[n1])
        assert (gb.num_graphs, gb.num_rows) == (g1 - g0, n1 - n0)
        assert torch.equal(gb.vrowptr, whole.vrowptr[2 * n0:2 * n1 + 1] - e0)
        assert torch.equal(gb.vcol, whole.vcol[e0:e1] - n0)
        assert np.array_equal(gb.graph_ptr.cpu().numpy(), gs.graph_ptr[g0:g1 + 1] - n0)
        host = GraphBatch(gs, "cpu", g0, g1)
        assert torch.equal(gb.vrowptr.cpu(), host.vrowptr) and torch.equal(gb.vcol.cpu(), host.vcol)
        moved = host.to(DEV)
        assert torch.equal(moved.vrowptr, gb.vrowptr) and torch.equal(moved.vcol, gb.vcol)


def test_train_index_of_a_graph_batch_equals_the_host_transpose():
    """the backward gather's index (desco_vcsr_transpose_sym) on the device-built arrays"""
    from desco_amd.batch import _transpose_index
    gs = GraphSet.from_edge_lists(random_family_graphs(7, 22))
    gb = GraphBatch(gs, DEV)
    ti = gb.train_index()
    t_rowptr, t_col = _transpose_index(gb.vrowptr.cpu().numpy(), gb.vcol.cpu().numpy(), gs.num_nodes)
    assert np.array_equal(ti["t_rowptr"].cpu().numpy(), t_rowptr)
    assert np.array_equal(ti["t_col"].cpu().numpy(), t_col)
    assert np.array_equal(ti["seg_id"].cpu().numpy(), gs.node_graph_ids())


def test_entry_point_refuses_bad_arguments():
    gs = GraphSet.from_edge_lists(CASES["K5"])
    rowptr, col = _graphset_device_csr(gs, DEV)
    with pytest.raises(ValueError):
        ops.graph_tconv_dev(rowptr, col, 0, 6, 0, 20)
    with pytest.raises(ValueError):
        ops.graph_tconv_dev(rowptr, col, 0, 5, 0, 21)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.graph_tconv_dev(rowptr.cpu(), col.cpu(), 0, 5, 0, 20)
