"""Host-side checks of the homogeneous ablation (ablation_gnns.py): the CPU restatement of the homogeneous model
(tests/homo_reference.py) against the oracle's hetero ``use_tconv=False`` path on the tied-weight state dict, the
``hetero_graph=False`` data surface (cache names, the 0/1 anchor feature, the refusals), the homogeneous model's state
dict and checkpoint round trip, and the per-type / per-relation accessors the weight packers read."""
import argparse
import os

import numpy as np
import pytest
import torch

import homo_reference as HR
from helpers import golden_graphs, neigh_args, standard_queries

from desco_amd import gnn_model as GM
from desco_amd.graphs import GraphSet
from desco_amd.lightning_model import NeighborhoodCountingModel
from desco_amd.partition import build_partition
from desco_amd.workload import NeighborhoodDataset, Workload
from oracle import model as OM
from oracle import partition as OP

FIVE_CYCLE = (6, [(3, 5), (5, 0), (0, 1), (1, 2), (2, 3)])


def homo_model(layer_num=2, hidden=64, seed=0, dropout=0.0, gain=1.3, **over):
    """A seeded homogeneous model, widened like helpers.make_models' (default nn.Linear init makes deep relu stacks
    collapse to constants)."""
    torch.manual_seed(seed)
    args = argparse.Namespace(**{**vars(neigh_args(layer_num=layer_num, hidden_dim=hidden, dropout=dropout)),
                                 "use_hetero": False, "use_tconv": False, "use_canonical": True, **over})
    nm = NeighborhoodCountingModel(1, hidden, args)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in nm.parameters():
            if p.dim() == 2:
                p.mul_(gain)
            else:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    return nm


@pytest.mark.parametrize("layer_num", [2, 8])
def test_restatement_equals_the_oracle_hetero_path_on_tied_weights(layer_num):
    """float64 on both sides: the two forms differ only in summation order, so they agree to rounding"""
    graphs = [FIVE_CYCLE] + golden_graphs(max_n=30)[:6]
    _, queries = standard_queries()
    neighs = HR.restricted_neighborhoods(graphs, 3)
    assert len(neighs) > 40
    nm = homo_model(layer_num)
    sd = {k: v.detach().double() for k, v in nm.state_dict().items()}
    torch.set_default_dtype(torch.float64)
    try:
        hb = HR.homo_batch([(nodes, es) for _, _, nodes, es in neighs])
        hb["node_feature"] = hb["node_feature"].double()
        qb = HR.homo_query_batch(queries)
        qb["node_feature"] = qb["node_feature"].double()
        emb_t, logits = HR.homo_logits(sd, hb, qb, layer_num)
        tied = HR.tied_hetero_state_dict(sd, layer_num)
        ob = OP.neighborhood_batch([(nodes, es) for _, _, nodes, es in neighs], tconv=False)
        ref_q = OM.base_gnn_hetero(tied, "emb_model_query", OP.query_batch(queries, tconv=False), ("union_node",),
                                   HR.QUERY_UNION, layer_num)
        ref_t = OM.base_gnn_hetero(tied, "emb_model", ob, OP.NODE_TYPES, HR.UNION_EDGE_TYPES, layer_num,
                                   feats={k: v.double() for k, v in HR.hetero_feats(ob).items()}, emulate_quirk=False)
        ref_logits = OM.head_logits(tied, ref_t, ref_q)
    finally:
        torch.set_default_dtype(torch.float32)
    assert float(ref_t.std(0).mean()) > 1e-3, "embeddings do not depend on the neighborhood"
    scale = float(ref_t.abs().max())
    assert float((emb_t - ref_t).abs().max()) <= 1e-10 * max(scale, 1.0)
    assert float((logits - ref_logits).abs().max()) <= 1e-10 * max(float(ref_logits.abs().max()), 1.0)
    # the anchor matters: without the feature the canonical rows would be count rows
    hb0 = dict(hb, node_feature=torch.zeros_like(hb["node_feature"]))
    assert float((HR.base_gnn_homo(sd, "emb_model", hb0, layer_num) - emb_t).abs().max()) > 1e-3


def test_partition_rows_maps_the_builder_layout_to_the_restatement():
    graphs = [FIVE_CYCLE] + golden_graphs(max_n=20)[:3]
    neighs = HR.restricted_neighborhoods(graphs, 2)
    part = build_partition(GraphSet.from_edge_lists(graphs), 2, restricted=True)
    assert part.neigh_index.tolist() == [[g, v] for g, v, _, _ in neighs]
    rows = HR.partition_rows(part)
    hb = HR.homo_batch([(nodes, es) for _, _, nodes, es in neighs])
    assert sorted(rows.tolist()) == list(range(part.num_rows))
    assert hb["node_feature"][rows, 0].tolist() == [0.0] * part.num_count + [1.0] * part.num_neigh
    gptr = np.concatenate([[0], np.cumsum([n for n, _ in graphs])])
    flat_ids = np.concatenate([np.asarray(nodes) + gptr[g] for g, _, nodes, _ in neighs])
    assert flat_ids[rows[:part.num_count]].tolist() == part.count_orig.tolist()


# ---- data surface ---------------------------------------------------------------------------------------------------
def test_homogeneous_dataset_cache_names_feature_and_refusals(tmp_path):
    graphs = [FIVE_CYCLE] + golden_graphs(max_n=20)[:4]
    gs = GraphSet.from_edge_lists(graphs)
    root = str(tmp_path / "nd")
    ds = NeighborhoodDataset(2, root, dataset=gs, hetero_graph=False)
    assert ds.processed_file_names == ["neighs_csr_depth_2_homo.npz", "neighs_index_depth_2_homo.npy",
                                       "neighs_indicator_depth_2_homo.npy"]
    assert sorted(os.listdir(os.path.join(root, "processed"))) == sorted(ds.processed_file_names)
    host = build_partition(gs, 2, restricted=True)
    assert ds.partition.restricted and np.array_equal(ds.partition.vcol, host.vcol)
    assert np.array_equal(ds.nx_neighs_index, host.neigh_index) and np.array_equal(ds.nx_neighs_indicator, host.indicator)
    # the hetero dataset of the same root keeps its own files and its own (larger) neighborhoods
    het = NeighborhoodDataset(2, root, dataset=gs, hetero_graph=True)
    assert het.processed_file_names[0] == "neighs_csr_depth_2.npz" and not het.partition.restricted
    assert het.partition.num_count > ds.partition.num_count
    # a second construction reads the cache and gives the same partition
    again = NeighborhoodDataset(2, root, dataset=gs, hetero_graph=False)
    assert again.partition_backend == "cache" and again.partition.restricted
    assert np.array_equal(again.partition.vrowptr, host.vrowptr) and np.array_equal(again.partition.vcol, host.vcol)
    # batches carry the anchor flag
    seen = 0
    for b in ds.batches(7):
        assert b.anchor_flag and b.input_dim == 1 and b.node_feature.shape == (b.num_rows, 1)
        assert b.node_feature[:, 0].tolist() == [0.0] * b.num_count + [1.0] * b.num_graphs
        assert b.node_feature_dict["count"].sum() == 0 and bool((b.node_feature_dict["canonical"] == 1).all())
        seen += b.num_graphs
    assert seen == len(ds) == host.num_neigh
    assert het.batch(0, 4).node_feature is None and not het.batch(0, 4).anchor_flag
    with pytest.raises(NotImplementedError, match=r"hetero_graph=False.*--use_node_feature"):
        NeighborhoodDataset(2, None, dataset=gs, hetero_graph=False, node_feat=True)
    with pytest.raises(NotImplementedError, match="quirk_batch"):
        NeighborhoodDataset(2, None, dataset=gs, hetero_graph=False, quirk_batch=4)


def test_workload_builds_the_homogeneous_datasets(tmp_path):
    gs = GraphSet.from_edge_lists(golden_graphs(max_n=20)[:5])
    w = Workload(gs, str(tmp_path / "w"), hetero_graph=False)
    w.canonical_count_truth = torch.arange(gs.num_nodes * 3, dtype=torch.float32).view(gs.num_nodes, 3)
    w.generate_pipeline_datasets(depth_neigh=4)
    nd = w.neighborhood_dataset
    assert nd.partition.restricted and not nd.hetero_graph
    assert os.path.exists(os.path.join(str(tmp_path / "w"), "NeighborhoodDataset", "processed", "neighs_csr_depth_4_homo.npz"))
    # the ground truth does not depend on the neighborhood definition: the kept nodes' rows, as for the hetero dataset
    assert torch.equal(nd.y, w.canonical_count_truth[torch.from_numpy(nd.nx_neighs_indicator)])
    b = nd.batch(0, 5)
    assert torch.equal(b.y, nd.y[:5]) and b.anchor_flag
    with pytest.raises(NotImplementedError, match=r"hetero_graph=False.*--use_node_feature"):
        Workload(GraphSet.from_edge_lists([FIVE_CYCLE], node_feat=np.eye(2, dtype=np.float32)[[0, 1, 0, 1, 0, 1]]),
                 None, hetero_graph=False, node_feat_len=2)


# ---- model surface --------------------------------------------------------------------------------------------------
def test_homogeneous_state_dict_and_checkpoint_round_trip(tmp_path):
    nm = homo_model(layer_num=3)
    keys = list(nm.state_dict())
    for m in ("emb_model", "emb_model_query"):
        assert f"{m}.gnn_core.pre_mp.0.weight" in keys and f"{m}.gnn_core.pre_mp.0.bias" in keys
        for l in range(3):
            assert f"{m}.gnn_core.convs.{l}.lin.weight" in keys and f"{m}.gnn_core.updates.{l}.bias" in keys
    assert not any("__" in k or ".count." in k or ".canonical." in k for k in keys)
    path = str(tmp_path / "homo.ckpt")
    nm.save_checkpoint(path)
    back = NeighborhoodCountingModel.load_from_checkpoint(path)
    assert back.emb_model.gnn_core.node_types is None and back.emb_model.gnn_core.is_homogeneous()
    assert back.args.use_hetero is False and back.args.use_canonical is True
    a, b = nm.state_dict(), back.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_accessors_return_the_one_shared_module():
    nm = homo_model(layer_num=2)
    core = nm.emb_model.gnn_core
    assert core.row_types() == ["count", "canonical"] and nm.emb_model_query.gnn_core.row_types() == ["union_node"]
    assert [len(core.slot_keys(t)) for t in ("count", "canonical", "union_node")] == [4, 2, 2]
    assert len(set(core.slot_keys("count"))) == 1                      # one relation: one weight, one bias
    for t in core.row_types():
        assert core.pre_lin(t) is core.pre_mp[0] and core.update(1, t) is core.updates[1]
        assert all(core.conv(0, k) is core.convs[0] for k in core.slot_keys(t))
    # the folded operands of the tied model equal those of the untied twin (pack_shmp: the packers' one folding)
    pk = GM.pack_shmp(nm.emb_model, bf16_planes=False)
    U, c = core.updates[0].weight, core.updates[0].bias
    W, b = core.convs[0].lin.weight, core.convs[0].lin.bias
    blk = (U[:, :64] @ W).t()
    want = torch.cat([blk] * 4 + [U[:, 64:].t()], 0)
    assert torch.allclose(pk["layers"][0]["count"]["wt"], want, atol=1e-6)
    assert torch.allclose(pk["layers"][0]["count"]["b"], U[:, :64] @ b + c, atol=1e-6)       # ONE bias
    assert torch.allclose(pk["layers"][0]["canonical"]["wt"], torch.cat([blk] * 2 + [U[:, 64:].t()], 0), atol=1e-6)
    # a hetero model keeps its per-type modules, and an unconverted hetero core is still refused
    het = NeighborhoodCountingModel(1, 64, neigh_args(layer_num=2))
    with pytest.raises(NotImplementedError, match="to_hetero"):
        het.emb_model.gnn_core.row_types()
    het.to_hetero_old(True, True)
    hc = het.emb_model.gnn_core
    assert hc.row_types() == ["count", "canonical"] and not hc.is_homogeneous()
    assert hc.pre_lin("count") is hc.pre_mp[0]["count"] and hc.update(0, "canonical") is hc.updates[0]["canonical"]


def test_set_queries_hetero_false_builds_zero_feature_queries():
    import networkx as nx
    nm = homo_model(layer_num=2)
    qs = [nx.path_graph(3), nx.cycle_graph(4)]
    for q in qs:
        for v in q.nodes:
            q.nodes[v]["feat"] = [1.0]
    nm.set_queries(None, queries=qs, hetero=False)
    assert nm.query_feat is None and nm.query_loader.node_feature is None
    nm.set_queries(None, queries=qs, hetero=True)
    assert nm.query_feat is not None and float(nm.query_feat.sum()) == 7.0
