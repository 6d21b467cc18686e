"""Neighborhood models of other widths than 64 on the GPU (the wide path): logits against the CPU oracle
at H in {32, 100, 128, 256}, the gossip model reading 128-wide query embeddings, the fused and un-fused wide layers
against each other, bit-identical repeats, and training gradients against torch autograd through the oracle."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from desco_amd import gnn_model as GM  # noqa: E402
from desco_amd import ops  # noqa: E402
from desco_amd.batch import GossipBatch, NeighborhoodBatch  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402
from desco_amd.partition import build_partition  # noqa: E402
from oracle import model as OM  # noqa: E402
from oracle import partition as OP  # noqa: E402

from helpers import (GOSSIP_GRAD_TOL, assert_counts_close, assert_grad_close, assert_logits_close,  # noqa: E402
                     assert_loss_close, cpu_sd, golden_graphs, report, standard_queries)
from test_neigh_width_host import width_models  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _models(h, tconv=True, seed=0):
    nm, gm = width_models(h, seed=seed, tconv=tconv, layer_num=8)
    qids, _ = standard_queries()
    nm, gm = nm.to(DEV), gm.to(DEV)
    nm.set_queries(qids)
    return nm, gm


def _logits_vs_oracle(nm, graphs, name, tconv=True):
    _, queries = standard_queries()
    gs = GraphSet.from_edge_lists(graphs)
    part = build_partition(gs, 4)
    _, _, neighs = OP.neighborhood_dataset(graphs, 4)
    sd = cpu_sd(nm)
    if tconv:
        ref = OM.neighborhood_logits(sd, OP.neighborhood_batch(neighs), OP.query_batch(queries), emulate_quirk=False)[0]
    else:
        union_types = (("count", "union", "canonical"), ("canonical", "union", "count"), ("count", "union", "count"))
        emb_q = OM.base_gnn_hetero(sd, "emb_model_query", OP.query_batch(queries, tconv=False), ("union_node",),
                                   (("union_node", "union", "union_node"),), 8)
        emb_t = OM.base_gnn_hetero(sd, "emb_model", OP.neighborhood_batch(neighs, tconv=False), OP.NODE_TYPES,
                                   union_types, 8, emulate_quirk=False)
        ref = OM.head_logits(sd, emb_t, emb_q)
    batch = NeighborhoodBatch(part, DEV)
    with torch.no_grad():
        got = nm._logits(batch, exp2=False)
    report(name, got, ref)
    assert_logits_close(name, got, ref)
    return batch, got


@pytest.mark.parametrize("h", [32, 100, 128, 256])
def test_wide_logits_vs_oracle(h):
    nm, _ = _models(h)
    assert nm.emb_model.is_wide()
    batch, got = _logits_vs_oracle(nm, golden_graphs(max_n=60), f"neigh_logits h={h}")
    qe = nm.get_query_emb()
    assert tuple(qe.shape) == (29, h)
    with torch.no_grad():
        emb = nm.graph_to_embed(batch)
    assert tuple(emb.shape) == (batch.num_graphs, h)


def test_wide_logits_hub_rows_and_union_edges():
    """h = 128 on a Syn_1827-shaped block: the dense 704-node graph (hub rows) beside golden graphs; and with
    use_tconv=False (one weight for both relation slots)."""
    import networkx as nx
    g = nx.gnm_random_graph(704, 704 * 12, seed=3)
    dense = (704, sorted((min(a, b), max(a, b)) for a, b in g.edges()))
    nm, _ = _models(128)
    _logits_vs_oracle(nm, golden_graphs(max_n=40)[:4] + [dense], "neigh_logits h=128 dense 704-node graph")
    nm, _ = _models(128, tconv=False)
    _logits_vs_oracle(nm, golden_graphs(max_n=60), "neigh_logits h=128 use_tconv=False", tconv=False)


@pytest.mark.parametrize("h", [128, 256])
def test_fused_and_unfused_wide_layers_agree(h):
    nm, _ = _models(h)
    graphs = golden_graphs(max_n=60)
    batch = NeighborhoodBatch(build_partition(GraphSet.from_edge_lists(graphs), 4), DEV)
    old = GM.SHMP_WIDE_FUSED
    try:
        with torch.no_grad():
            GM.SHMP_WIDE_FUSED = True
            fused = nm._logits(batch, exp2=False).clone()
            GM.SHMP_WIDE_FUSED = False
            unfused = nm._logits(batch, exp2=False).clone()
    finally:
        GM.SHMP_WIDE_FUSED = old
    assert_logits_close(f"fused vs un-fused wide layers h={h}", fused, unfused)


def test_wide_layer_kernel_is_bit_identical_across_launches():
    nm, _ = _models(128)
    graphs = golden_graphs(max_n=60)
    batch = NeighborhoodBatch(build_partition(GraphSet.from_edge_lists(graphs), 4), DEV)
    pk = nm.emb_model.packed()
    e = pk["layers"][1]["count"]
    g = torch.Generator().manual_seed(5)
    x = torch.relu(torch.randn(batch.num_rows, 128, generator=g)).to(DEV)
    outs = []
    for _ in range(50):
        out = torch.empty_like(x)
        ops.shmp_layer_wide(x, batch.vrowptr, batch.vcol, 4, 0, batch.num_count, 4, e["w16"], e["b"], out=out)
        outs.append(out[:batch.num_count])
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    # un-fused cross-check of the same launch: gather + f16x3 GEMM
    agg = ops.csr_gather_sum_wide(x, batch.vrowptr, batch.vcol, batch.num_rows, 4)
    ref = ops.gemm_f16x3(agg[:batch.num_count], e["w16"], e["b"], a2=x[:batch.num_count], act=ops.ACT_RELU)
    assert_logits_close("wide layer kernel vs gather + GEMM", outs[0], ref, tol=1e-5)


def test_gossip_with_128_wide_query_embeddings_vs_oracle():
    from desco_amd.pipeline import InferencePipeline
    nm, gm = _models(128)
    _, queries = standard_queries()
    graphs = golden_graphs(max_n=60)
    gs = GraphSet.from_edge_lists(graphs)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(gs.num_nodes, len(queries), generator=g) * 30
    x[torch.rand(gs.num_nodes, generator=g) < 0.2] = 0
    qemb = nm.get_query_emb()
    gm.set_query_emb(qemb)
    batch = GossipBatch(gs, DEV, x=x)
    got = gm.graph_to_count(batch)
    ref = OM.gossip_graph_to_count(cpu_sd(gm), x, batch.edge_index.numpy(), qemb.cpu(), 2)
    assert_logits_close("gossip correction emb_channels=128", got.cpu() - x, ref - x, tol=2e-5)
    ref = OM.reference_pipeline(cpu_sd(nm), cpu_sd(gm), graphs, queries, emulate_quirk=False)
    pipe = InferencePipeline(nm, gm, gs, depth=4, device=DEV)
    out = pipe.run()
    for k in ("neigh_count", "node_count", "graph_neigh_count", "graph_gossip_count"):
        assert_counts_close(f"{k} h=128", out[k], ref[k])
    again = pipe.run()
    for k in ("neigh_count", "graph_gossip_count"):
        assert torch.equal(torch.as_tensor(out[k]), torch.as_tensor(again[k])), k


def test_gossip_training_with_128_wide_query_embeddings():
    nm, gm = _models(128)
    _, queries = standard_queries()
    graphs = golden_graphs(max_n=41)[:10]
    gs = GraphSet.from_edge_lists(graphs)
    g = torch.Generator().manual_seed(2)
    x = torch.rand(gs.num_nodes, len(queries), generator=g) * 20
    y = torch.floor(x + torch.rand(x.shape, generator=g) * 4)
    qemb = nm.get_query_emb().detach()
    gm.set_query_emb(qemb)
    batch = GossipBatch(gs, DEV, x=x, y=y)
    gm.zero_grad()
    loss = gm.train_forward(batch, 0)
    loss.backward()
    sd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in gm.state_dict().items()}
    ref_loss = OM.gossip_loss(sd, x, y, batch.edge_index.numpy(), qemb.cpu(), 2)
    ref_loss.backward()
    assert_loss_close("gossip train loss emb_channels=128", loss.detach(), ref_loss.detach())
    worst = 0.0
    for name, p in gm.named_parameters():
        ref = sd[name].grad
        if ref is None or float(ref.abs().max()) == 0.0:
            continue
        worst = max(worst, assert_grad_close(name, p.grad, ref, tol=GOSSIP_GRAD_TOL))
    print(f"[gate] gossip gradients emb_channels=128: worst {worst:.2e} (gate {GOSSIP_GRAD_TOL:.0e})")


@pytest.mark.parametrize("h", [32, 128])
def test_wide_training_loss_and_gradients_vs_oracle(h):
    nm, _ = _models(h)
    _, queries = standard_queries()
    graphs = golden_graphs(max_n=41)[:14]
    part = build_partition(GraphSet.from_edge_lists(graphs), 4)
    g = torch.Generator().manual_seed(4)
    y = torch.floor(torch.rand(part.num_neigh, len(queries), generator=g) ** 3 * 40)
    batch = NeighborhoodBatch(part, DEV, y=y)
    nm.zero_grad()
    loss = nm.train_forward(batch, 0)
    loss.backward()
    sd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in nm.state_dict().items()}
    _, _, neighs = OP.neighborhood_dataset(graphs, 4)
    ref_loss = OM.neighborhood_loss(sd, OP.neighborhood_batch(neighs), OP.query_batch(queries), y, emulate_quirk=False)
    ref_loss.backward()
    assert_loss_close(f"wide train loss h={h}", loss.detach(), ref_loss.detach())
    worst = 0.0
    for name, p in nm.named_parameters():
        ref = sd[name].grad
        if ref is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert p.grad is not None and tuple(p.grad.shape) == tuple(p.shape), name
        worst = max(worst, assert_grad_close(name, p.grad, ref))
    print(f"[gate] wide gradients h={h}: worst relative error {worst:.2e}")


def test_wide_adam_steps_reduce_loss_with_dropout():
    nm, _ = _models(128)
    nm.emb_model.gnn_core.dropout = nm.emb_model_query.gnn_core.dropout = 0.1
    nm.train()
    _, queries = standard_queries()
    graphs = golden_graphs(max_n=41)[:14]
    part = build_partition(GraphSet.from_edge_lists(graphs), 4)
    g = torch.Generator().manual_seed(4)
    y = torch.floor(torch.rand(part.num_neigh, len(queries), generator=g) ** 3 * 40)
    batch = NeighborhoodBatch(part, DEV, y=y)
    opt = torch.optim.Adam(nm.parameters(), lr=1e-3)
    losses = []
    for _ in range(8):
        opt.zero_grad()
        loss = nm.train_forward(batch, 0)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print(f"[gate] wide Adam steps (dropout 0.1): losses {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert all(map(lambda v: v == v, losses)) and losses[-1] < losses[0]


def test_wide_pipeline_eager_and_captured_replay_are_bit_identical():
    from desco_amd.pipeline import InferencePipeline
    nm, gm = _models(128)
    gs = GraphSet.from_edge_lists(golden_graphs(max_n=60))
    pipe = InferencePipeline(nm, gm, gs, depth=4, device=DEV)
    eager = {k: v.clone() for k, v in pipe.run().items()}
    pipe.capture()
    rep = pipe.run_graph()
    rep2 = {k: v.clone() for k, v in rep.items()}
    rep = pipe.run_graph()
    torch.cuda.synchronize()
    keys = ("neigh_count", "node_count", "graph_gossip_count")
    same = all(torch.equal(eager[k], rep[k]) and torch.equal(eager[k], rep2[k]) for k in keys)
    print(f"[replay] h=128 pipeline: eager == two captured replays bit for bit: {same}")
    assert same


def test_invalidate_caches_drops_the_wide_caches():
    """An update that does not bump tensor._version (a replayed optimizer step) is followed by invalidate_caches():
    the padded query embeddings and the head operands must be rebuilt from the new values."""
    nm, _ = _models(128)
    batch = NeighborhoodBatch(build_partition(GraphSet.from_edge_lists(golden_graphs(max_n=60)), 4), DEV)
    with torch.no_grad():
        before = nm._logits(batch, exp2=False).clone()
        for m in (nm.count_model, nm.emb_model_query, nm.emb_model):
            for p in m.parameters():
                p.data.mul_(0.9)           # (through .data: the parameter's own version counter does not move)
        nm.invalidate_caches()
        after = nm._logits(batch, exp2=False).clone()
    fresh, _ = _models(128)
    fresh.load_state_dict(nm.state_dict())
    with torch.no_grad():
        ref = fresh._logits(batch, exp2=False)
    assert not torch.equal(before, after)
    assert torch.equal(after, ref)


def test_graph_capture_refuses_wide_models():
    from desco_amd.trainer import Trainer
    nm, _ = _models(128)
    with pytest.raises(NotImplementedError, match="--neigh_hidden_dim"):
        Trainer(max_epochs=2, graph_capture=True).fit(nm, None)


@pytest.mark.parametrize("h", [32, 128])
def test_wide_training_with_dropout_vs_oracle_with_the_same_masks(h):
    """--neigh_dropout 0.1 at width h: one step's loss and gradients against autograd through the oracle fed with the
    pass's own factors -- layer l of a model: site 2 l of its key over all its rows (count rows, then canonical), post_mp.1:
    POST_DROP_SITE; the query model draws the first key, the target model the second."""
    p = 0.1
    nm, _ = _models(h)
    for m in (nm.emb_model, nm.emb_model_query):
        m.gnn_core.dropout, m.post_mp[1].p = p, p
    _, queries = standard_queries()
    graphs = golden_graphs(max_n=41)[:10]
    part = build_partition(GraphSet.from_edge_lists(graphs), 4)
    _, _, neighs = OP.neighborhood_dataset(graphs, 4)
    g = torch.Generator().manual_seed(9)
    y = torch.floor(torch.rand(part.num_neigh, len(queries), generator=g) ** 3 * 40)
    batch = NeighborhoodBatch(part, DEV, y=y)
    seed = 31337
    ops.manual_seed(seed, step=10)
    nm.train()
    nm.zero_grad()
    loss = nm.train_forward(batch, 0)
    loss.backward()
    torch.cuda.synchronize()
    assert ops.rng_state(DEV).cpu().tolist() == [seed, 12]
    kq = torch.tensor([seed, 10], dtype=torch.int64, device=DEV)
    kt = torch.tensor([seed, 11], dtype=torch.int64, device=DEV)
    Nc, B, nq, wp = batch.num_count, batch.num_graphs, sum(n for n, _ in queries), GM.padded_width(h)

    def fac(key, site, rows):
        return ops.dropout_mask(ops.DropSite(key, site, p), rows, wp).cpu()[:, :h]
    lt = [fac(kt, GM.wide_layer_drop_site(l), Nc + B) for l in range(8)]
    masks_t = ([{"count": m[:Nc], "canonical": m[Nc:]} for m in lt], fac(kt, GM.POST_DROP_SITE, B))
    masks_q = ([{"union_node": fac(kq, GM.wide_layer_drop_site(l), nq)} for l in range(8)],
               fac(kq, GM.POST_DROP_SITE, len(queries)))
    sd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in nm.state_dict().items()}
    ob, qb = OP.neighborhood_batch(neighs), OP.query_batch(queries)
    ref_loss = OM.neighborhood_loss(sd, ob, qb, y, emulate_quirk=False, masks_t=masks_t, masks_q=masks_q)
    ref_loss.backward()
    assert_loss_close(f"wide train loss h={h}, dropout {p}", loss.detach(), ref_loss.detach())
    # the masks matter: without them the oracle is much further from the step than with them
    plain = OM.neighborhood_loss({k: v.detach() for k, v in sd.items()}, ob, qb, y, emulate_quirk=False)
    d_plain, d_masked = abs(float(plain) - float(loss)), abs(float(ref_loss) - float(loss))
    print(f"[gate] |loss - oracle|: {d_masked:.2e} with the masks, {d_plain:.2e} without")
    assert d_plain > 20 * max(d_masked, 1e-7 * abs(float(loss)))
    worst, checked = 0.0, 0
    for name, prm in nm.named_parameters():
        ref = sd[name].grad
        if ref is None or float(ref.abs().max()) == 0.0:
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, name
            continue
        worst = max(worst, assert_grad_close(name, prm.grad, ref))
        checked += 1
    print(f"[gate] wide gradients h={h} dropout {p}: worst relative error {worst:.2e} over {checked} tensors")
    assert checked > 150


def test_main_trains_predicts_and_writes_artifacts_at_width_128(tmp_path):
    import argparse
    import numpy as np
    import main as driver
    from desco_amd import config
    from desco_amd.data import STANDARD_QUERY_IDS
    from test_main_gpu import _write_tu
    root = str(tmp_path / "data")
    _write_tu(root, "TOY", golden_graphs(max_n=30))
    ap = argparse.ArgumentParser()
    config.parse_optimizer(ap)
    config.parse_neighborhood(ap)
    config.parse_gossip(ap)
    args = ap.parse_args(["--train_dataset", "TOY_train", "--valid_dataset", "TOY_val", "--test_dataset", "TOY_test",
                          "--neigh_hidden_dim", "128", "--neigh_epoch_num", "1", "--gossip_epoch_num", "1",
                          "--neigh_batch_size", "64", "--gossip_batch_size", "4",
                          "--neigh_model_path", str(tmp_path / "ckpt_n"), "--gossip_model_path", str(tmp_path / "ckpt_g"),
                          "--train_neigh", "--train_gossip", "--test_gossip", "--output_dir", str(tmp_path / "out")])
    an, ag, ao = config.split_namespaces(args)
    assert an.hidden_dim == 128
    rep = driver.main(an, ag, ao, train_neighborhood=True, train_gossip=True, test_gossip=True,
                      atlas_query_ids=STANDARD_QUERY_IDS, output_dir=str(tmp_path / "out"), data_root=root)
    out = tmp_path / "out"
    for f in ["neighborhood_graphlet_TOY_test.csv", "gossip_graphlet_TOY_test.csv", "graphlet_count_TOY_test.csv",
              "analyze_results_TOY_test.txt"]:
        assert (out / f).exists(), f
    assert all(np.isfinite(rep["graphlet_mae_gossip"])) and all(np.isfinite(rep["graphlet_mae_neighborhood"]))
    rep2 = driver.main(an, ag, ao, train_neighborhood=False, train_gossip=False, test_gossip=True,
                       neighborhood_checkpoint=str(tmp_path / "ckpt_n" / "last.ckpt"),
                       gossip_checkpoint=str(tmp_path / "ckpt_g" / "last.ckpt"),
                       atlas_query_ids=STANDARD_QUERY_IDS, output_dir=str(tmp_path / "out2"), data_root=root)
    assert all(np.isfinite(rep2["graphlet_mae_gossip"]))


def test_lightning_layout_checkpoint_at_width_128_loads_and_predicts(tmp_path):
    from desco_amd.lightning_model import NeighborhoodCountingModel
    from test_ckpt_reader import _write_lightning_like
    nm, _ = width_models(128, layer_num=8)
    path = str(tmp_path / "neigh128.ckpt")
    _write_lightning_like(path, nm)
    nm2 = NeighborhoodCountingModel.load_from_checkpoint(path)
    assert nm2.hidden_dim == 128 and nm2.emb_model.is_wide()
    qids, _ = standard_queries()
    batch = NeighborhoodBatch(build_partition(GraphSet.from_edge_lists(golden_graphs(max_n=60)), 4), DEV)
    counts = []
    for m in (nm, nm2):
        m = m.to(DEV)
        m.set_queries(qids)
        counts.append(m.graph_to_count(batch))
    assert torch.equal(counts[0], counts[1])


_TRACE_SCRIPT = r"""
import sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import torch
from desco_amd.batch import NeighborhoodBatch
from desco_amd.graphs import GraphSet
from desco_amd.partition import build_partition
from helpers import golden_graphs, standard_queries
from test_neigh_width_host import width_models
nm, _ = width_models(128, layer_num=8)
nm = nm.cuda().eval()
nm.set_queries(standard_queries()[0])
batch = NeighborhoodBatch(build_partition(GraphSet.from_edge_lists(golden_graphs(max_n=60)), 4), "cuda")
with torch.no_grad():
    for _ in range(2 + int(sys.argv[1])):         # two warm-up passes (caches), then the counted ones
        nm._logits(batch, exp2=True)
torch.cuda.synchronize()
"""


def test_warm_wide_pass_launches_only_this_librarys_kernels(tmp_path):
    """rocprofv3 --kernel-trace --stats of 2 and of 6 warm h = 128 inference passes: every kernel whose call count grows
    with the passes is one of this library's (set-up kernels -- folding, padding -- have the same count in both)."""
    import csv
    import glob
    import shutil
    import subprocess
    assert shutil.which("rocprofv3"), "rocprofv3 not found"
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "trace_pass.py"
    script.write_text(_TRACE_SCRIPT.format(repo=repo, tests=os.path.join(repo, "tests")))
    counts = {}
    for k in (2, 6):
        d = tmp_path / f"s{k}"
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(d), "--",
                            sys.executable, str(script), str(k)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        files = glob.glob(str(d / "**" / "*kernel_stats.csv"), recursive=True)
        assert files, f"no kernel stats for {k} passes"
        tab = {}
        for f in files:
            for r in csv.DictReader(open(f)):
                tab[r["Name"]] = tab.get(r["Name"], 0) + int(r["Calls"])
        counts[k] = tab
    a, b = counts[2], counts[6]
    grow = {n: (a.get(n, 0), c) for n, c in b.items() if c != a.get(n, 0)}
    foreign = [n for n in grow if "desco" not in n]
    print(f"[trace] h=128 pass: {len(grow)} kernels grow with the passes, "
          f"{sum(v[1] - v[0] for v in grow.values()) // 4} launches per pass; foreign: {foreign}")
    assert grow and not foreign
