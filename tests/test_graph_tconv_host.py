"""The host routine behind ``GraphBatch`` (desco_graph_tconv: the triangle / tride typed CSR of whole graphs) against the
construction ``QueryBatch`` uses (dense ``tconv_split`` + sort) and against a brute-force common-neighbour test, and the
model surface of the ablation without canonical partition (``to_hetero_wo_canonical``, checkpoints) -- all on the CPU."""
import argparse

import numpy as np
import pytest
import torch

from desco_amd import ops
from desco_amd.batch import GraphBatch, QueryBatch
from desco_amd.graphs import GraphSet
from desco_amd.lightning_model import NeighborhoodCountingModel
from helpers import neigh_args, random_family_graphs

H = 64

TRIANGLE = (3, [(0, 1), (1, 2), (0, 2)])
K5 = (5, [(a, b) for a in range(5) for b in range(a + 1, 5)])
C5 = (5, [(v, (v + 1) % 5) for v in range(5)])
PATH_CHORD = (6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (1, 3)])

CASES = {
    "empty set": [],
    "single node": [(1, [])],
    "single edge": [(2, [(0, 1)])],
    "triangle": [TRIANGLE],
    "K5": [K5],
    "C5": [C5],
    "path with one chord": [PATH_CHORD],
    "two graphs": [PATH_CHORD, K5],
    "isolated nodes between graphs": [(3, []), TRIANGLE, (2, []), C5],
    "random families": random_family_graphs(11, 44),
}


def brute_force(graphs):
    """(vrowptr, vcol) from the definition: per row, per neighbour in ascending order, is there a common neighbour?"""
    gp = np.concatenate([[0], np.cumsum([n for n, _ in graphs])]).astype(np.int64)
    adj = [set() for _ in range(int(gp[-1]))]
    for g, (n, edges) in enumerate(graphs):
        for a, b in edges:
            if a != b:
                adj[a + gp[g]].add(b + gp[g])
                adj[b + gp[g]].add(a + gp[g])
    vrowptr, vcol = [0], []
    for v, nb in enumerate(adj):
        tri = [s for s in sorted(nb) if adj[s] & nb]
        tride = [s for s in sorted(nb) if not (adj[s] & nb)]
        vcol += tri
        vrowptr.append(len(vcol))
        vcol += tride
        vrowptr.append(len(vcol))
    return np.array(vrowptr, dtype=np.int32), np.array(vcol, dtype=np.int32)


def check_invariants(graphs, vrowptr, vcol):
    gs = GraphSet.from_edge_lists(graphs)
    assert vrowptr.dtype == np.int32 and vcol.dtype == np.int32
    assert len(vrowptr) == 2 * gs.num_nodes + 1 and vrowptr[0] == 0
    assert (np.diff(vrowptr) >= 0).all() and vrowptr[-1] == len(vcol) == len(gs.col)
    gid = gs.node_graph_ids()
    for r in range(2 * gs.num_nodes):
        run = vcol[vrowptr[r]:vrowptr[r + 1]]
        assert (np.diff(run) > 0).all(), f"(row, slot) {divmod(r, 2)} does not ascend"
        assert (gid[run] == gid[r // 2]).all(), f"row {r // 2} has a source outside its graph"


@pytest.mark.parametrize("name", list(CASES))
def test_host_routine_equals_the_query_batch_construction_and_brute_force(name):
    graphs = CASES[name]
    gs = GraphSet.from_edge_lists(graphs)
    vrowptr, vcol = ops.graph_tconv_host(gs.rowptr, gs.col, 0, gs.num_nodes)
    check_invariants(graphs, vrowptr, vcol)
    ref_ptr, ref_col = brute_force(graphs)
    assert np.array_equal(vrowptr, ref_ptr) and np.array_equal(vcol, ref_col)
    qb = QueryBatch(graphs, "cpu")
    assert np.array_equal(vrowptr, qb.vrowptr.numpy()) and np.array_equal(vcol, qb.vcol.numpy())
    gb = GraphBatch(gs, "cpu")
    assert gb.slots == 2 and gb.num_graphs == len(graphs) and gb.num_rows == gs.num_nodes
    assert torch.equal(gb.vrowptr, qb.vrowptr) and torch.equal(gb.vcol, qb.vcol)
    assert torch.equal(gb.graph_ptr, qb.graph_ptr)
    assert np.array_equal(gb._seg_ptr_host(), qb._seg_ptr_host())


def test_triangle_and_tride_slots_of_known_graphs():
    for graphs, ntri in (([TRIANGLE], 6), ([K5], 20), ([C5], 0), ([PATH_CHORD], 6), ([(2, [(0, 1)])], 0)):
        gs = GraphSet.from_edge_lists(graphs)
        vrowptr, _ = ops.graph_tconv_host(gs.rowptr, gs.col, 0, gs.num_nodes)
        assert int((vrowptr[1::2] - vrowptr[:-1:2]).sum()) == ntri


def test_a_graph_range_is_the_slice_of_the_whole_set_rebased():
    graphs = random_family_graphs(5, 30)
    gs = GraphSet.from_edge_lists(graphs)
    whole_ptr, whole_col = ops.graph_tconv_host(gs.rowptr, gs.col, 0, gs.num_nodes)
    for g0, g1 in ((0, 1), (3, 11), (11, 11), (20, len(graphs))):
        gb = GraphBatch(gs, "cpu", g0, g1)
        n0, n1 = int(gs.graph_ptr[g0]), int(gs.graph_ptr[g1])
        e0, e1 = int(gs.rowptr[n0]), int(gs.rowptr[n1])
        assert gb.num_graphs == g1 - g0 and gb.num_rows == n1 - n0
        assert np.array_equal(gb.vrowptr.numpy(), whole_ptr[2 * n0:2 * n1 + 1] - e0)
        assert np.array_equal(gb.vcol.numpy(), whole_col[e0:e1] - n0)
        assert np.array_equal(gb.graph_ptr.numpy(), gs.graph_ptr[g0:g1 + 1] - n0)
        sub = GraphBatch(gs.subset(g0, g1), "cpu")
        assert torch.equal(sub.vrowptr, gb.vrowptr) and torch.equal(sub.vcol, gb.vcol)


def test_host_routine_does_not_depend_on_the_thread_count():
    gs = GraphSet.from_edge_lists(random_family_graphs(3, 60))
    a = ops.graph_tconv_host(gs.rowptr, gs.col, 0, gs.num_nodes, num_threads=1)
    b = ops.graph_tconv_host(gs.rowptr, gs.col, 0, gs.num_nodes, num_threads=7)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_graph_batch_features_truth_and_argument_checks():
    graphs = [TRIANGLE, C5]
    feat = np.arange(16, dtype=np.float32).reshape(8, 2)
    gs = GraphSet.from_edge_lists(graphs, node_feat=feat)
    y = torch.arange(6.0).reshape(2, 3)
    gb = GraphBatch(gs, "cpu", node_feature=True, y=y)
    assert gb.input_dim == 2 and torch.equal(gb.node_feature, torch.from_numpy(feat)) and torch.equal(gb.y, y)
    assert gb.to("cpu") is gb
    part = GraphBatch(gs, "cpu", 1, 2, node_feature=True)
    assert torch.equal(part.node_feature, torch.from_numpy(feat[3:]))
    assert GraphBatch(gs, "cpu").node_feature is None
    with pytest.raises(ValueError):
        GraphBatch(gs, "cpu", 1, 3)
    with pytest.raises(ValueError):
        GraphBatch(gs, "cpu", node_feature=torch.zeros(5, 2))
    with pytest.raises(ValueError):
        GraphBatch(GraphSet.from_edge_lists(graphs), "cpu", node_feature=True)
    with pytest.raises(ValueError):
        ops.graph_tconv_host(gs.rowptr, gs.col, 4, 9)


# ---- model surface -------------------------------------------------------------------------------------------------
def wo_canonical_args(**over):
    return neigh_args(use_canonical=False, **over)


@pytest.mark.parametrize("tconv", [True, False])
def test_state_dict_of_the_model_without_canonical_partition(tconv):
    L = 3
    nm = NeighborhoodCountingModel(1, H, wo_canonical_args(layer_num=L, use_tconv=tconv))
    assert nm.to_hetero_wo_canonical(tconv, tconv) is nm
    sd = nm.state_dict()
    rels = ("union_triangle", "union_tride") if tconv else ("union",)
    for m in ("emb_model", "emb_model_query"):
        core = getattr(nm, m).gnn_core
        assert core.node_types == ["union_node"]
        assert core.edge_types == [("union_node", r, "union_node") for r in rels]
        want = {f"{m}.gnn_core.pre_mp.0.union_node.weight": (H, 1), f"{m}.gnn_core.pre_mp.0.union_node.bias": (H,)}
        for l in range(L):
            for r in rels:
                want[f"{m}.gnn_core.convs.{l}.union_node__{r}__union_node.lin.weight"] = (H, H)
                want[f"{m}.gnn_core.convs.{l}.union_node__{r}__union_node.lin.bias"] = (H,)
            want[f"{m}.gnn_core.updates.{l}.union_node.weight"] = (H, 2 * H)
            want[f"{m}.gnn_core.updates.{l}.union_node.bias"] = (H,)
        got = {k: tuple(v.shape) for k, v in sd.items() if k.startswith(m + ".gnn_core.")}
        assert got == want
    # both models have the same keys up to their prefix: the target model has the query model's shape
    strip = lambda p: sorted(k[len(p):] for k in sd if k.startswith(p))          # noqa: E731
    assert strip("emb_model.") == strip("emb_model_query.")
    assert not any("count" in k.split(".")[-3] or "canonical" in k for k in sd if "gnn_core" in k)
    with pytest.raises(RuntimeError, match="already heterogeneous"):
        nm.to_hetero_wo_canonical(tconv, tconv)


@pytest.mark.parametrize("tconv", [True, False])
def test_checkpoint_without_canonical_partition_loads_with_single_type_cores(tmp_path, tconv):
    torch.manual_seed(2)
    nm = NeighborhoodCountingModel(1, H, wo_canonical_args(layer_num=2, use_tconv=tconv))
    nm.to_hetero_wo_canonical(tconv, tconv)
    path = str(tmp_path / "wo_canonical.ckpt")
    nm.save_checkpoint(path)
    back = NeighborhoodCountingModel.load_from_checkpoint(path)
    assert back.emb_model.gnn_core.node_types == ["union_node"]
    assert back.emb_model_query.gnn_core.node_types == ["union_node"]
    assert (back.tconv_target, back.tconv_query) == (tconv, tconv)
    a, b = nm.state_dict(), back.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_checkpoint_with_canonical_partition_loads_as_before(tmp_path):
    torch.manual_seed(3)
    for args in (neigh_args(layer_num=2), neigh_args(layer_num=2, use_canonical=True)):   # absent = canonical
        nm = NeighborhoodCountingModel(1, H, args).to_hetero_old(True, True)
        path = str(tmp_path / "canonical.ckpt")
        nm.save_checkpoint(path)
        back = NeighborhoodCountingModel.load_from_checkpoint(path)
        assert back.emb_model.gnn_core.node_types == ["count", "canonical"]
        assert "emb_model.gnn_core.convs.0.count__union_triangle__canonical.lin.weight" in back.state_dict()
        assert back.emb_model_query.gnn_core.node_types == ["union_node"]
        a, b = nm.state_dict(), back.state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_a_homogeneous_checkpoint_stays_homogeneous(tmp_path):
    nm = NeighborhoodCountingModel(1, H, argparse.Namespace(**{**vars(neigh_args(layer_num=2)), "use_hetero": False,
                                                              "use_canonical": False}))
    path = str(tmp_path / "homo.ckpt")
    nm.save_checkpoint(path)
    assert NeighborhoodCountingModel.load_from_checkpoint(path).emb_model.gnn_core.node_types is None


# ---- data surface --------------------------------------------------------------------------------------------------
def test_workload_hands_out_whole_graph_batches_with_the_reference_truth():
    """canonical_to_graphlet_truth = per-graph sums; the dataset's y is log2(sum + 1) (the reference stores the
    logarithm, workload.py:829-831); the loader's batches are GraphBatches over consecutive graph ranges."""
    from desco_amd.lightning_data import LightningDataLoader
    from desco_amd.transforms import ToTconvHetero
    from desco_amd.workload import WoCanonicalDataset, Workload
    graphs = random_family_graphs(2, 10)
    gs = GraphSet.from_edge_lists(graphs)
    w = Workload(gs, root=None)
    with pytest.raises(RuntimeError, match="canonical_to_graphlet_truth"):
        w.generate_wo_canonical_dataset()
    g = torch.Generator().manual_seed(0)
    truth = torch.randint(0, 50, (gs.num_nodes, 4), generator=g)
    sums = w.canonical_to_graphlet_truth(truth)
    assert sums.dtype == truth.dtype and sums.shape == (gs.num_graphs, 4)
    for i in range(gs.num_graphs):
        assert torch.equal(sums[i], truth[gs.graph_ptr[i]:gs.graph_ptr[i + 1]].sum(0))
    ds = w.generate_wo_canonical_dataset(transform=ToTconvHetero())
    assert ds is w.wo_canonical_dataset and isinstance(ds, WoCanonicalDataset) and len(ds) == gs.num_graphs
    assert torch.equal(ds.y, torch.log2(sums + 1).float())
    batches = list(LightningDataLoader(test_dataset=ds, batch_size=4).test_dataloader())
    assert [b.num_graphs for b in batches] == [4, 4, gs.num_graphs - 8]
    whole = GraphBatch(gs, "cpu")
    for k, b in enumerate(batches):
        assert isinstance(b, GraphBatch) and b.node_feature is None and b.slots == 2
        assert torch.equal(b.y, ds.y[4 * k:4 * k + 4])
        n0, e0 = int(gs.graph_ptr[4 * k]), int(gs.rowptr[gs.graph_ptr[4 * k]])
        assert torch.equal(b.vcol, whole.vcol[e0:e0 + b.vcol.numel()] - n0)
    with pytest.raises(NotImplementedError):
        w.generate_wo_canonical_dataset(transform=lambda d: d)
