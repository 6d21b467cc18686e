"""Gossip models of any depth (--gossip_layer_num != 2) on the GPU: the depth-L inference path (layer 0 in closed
form, L - 1 launches of desco_gossip_layer_f16x3_f32, the post_mp tail) against the CPU oracle at the reference's
semantics, on the golden graphs, a Syn_1827-shaped block with a hub and the dense 704-node graph, and more than 64
queries; bit-identical repeats of the layer kernel and of a captured InferencePipeline replay; the depth-L training
pass (autograd.GossipTrunkDeep) against torch autograd through the oracle, with and without dropout; a captured
Trainer against the eager one; main.py end to end at --gossip_layer_num 3.  Every gate prints what it measured."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from desco_amd import autograd as AG  # noqa: E402
from desco_amd import gnn_model as GM  # noqa: E402
from desco_amd import ops  # noqa: E402
from desco_amd.batch import GossipBatch  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402
from oracle import model as OM  # noqa: E402

from helpers import (GOSSIP_GRAD_TOL, LOGIT_TOL, assert_counts_close, assert_grad_close, assert_logits_close,  # noqa: E402
                     assert_loss_close, cpu_sd, gossip_args, golden_graphs, make_models, report, standard_queries)

DEV = "cuda"


def gossip_model(L, seed=0, gain=1.4, dropout=0.0):
    """GossipCountingModel with L GossipConv layers, seeded and widened as helpers.make_models does."""
    from desco_amd.lightning_model import GossipCountingModel
    torch.manual_seed(seed)
    gm = GossipCountingModel(1, 64, gossip_args(layer_num=L, dropout=dropout), emb_channels=64,
                             input_pattern_emb=True)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for _, p in gm.named_parameters():
            if p.dim() == 2:
                p.mul_(gain)
            else:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    return gm.to(DEV)


@pytest.fixture(scope="module")
def nm():
    nm, _ = make_models(seed=0)
    qids, _ = standard_queries()
    nm = nm.to(DEV)
    nm.set_queries(qids)
    return nm


def golden_inputs(Q):
    gs = GraphSet.from_edge_lists(golden_graphs(max_n=60))
    g = torch.Generator().manual_seed(1)
    x = torch.rand(gs.num_nodes, Q, generator=g) * 30
    x[torch.rand(gs.num_nodes, generator=g) < 0.2] = 0
    return gs, x


def syn_hub_graphs():
    """Syn_1827-shaped block cut as tests/test_model_gpu.py::test_heavy_tailed_shapes cuts it: the four largest graphs
    of at most 160 nodes plus the dense 704-node graph (hub rows with hundreds of neighbours)."""
    from desco_amd import synthetic
    full = synthetic.syn_1827_shaped(60)
    sizes = np.diff(full.graph_ptr)
    keep = [g for g in np.argsort(sizes)[::-1] if sizes[g] <= 160][:4]
    keep.append(int(np.argsort(sizes)[::-1][1]))
    return GraphSet.from_edge_lists([full.edge_lists()[g] for g in sorted(keep)])


def corrections(gm, batch, x, qemb, L):
    gm.set_query_emb(qemb)
    with torch.no_grad():
        got = gm.graph_to_count(batch).cpu() - x
    ref = OM.gossip_graph_to_count(cpu_sd(gm), x, batch.edge_index.numpy(), qemb.cpu(), layer_num=L) - x
    return got, ref


@pytest.mark.parametrize("L,tol", [(1, 2e-5), (3, 2e-5), (4, LOGIT_TOL)])
def test_deep_gossip_inference_vs_oracle(nm, L, tol):
    gm = gossip_model(L)
    qemb = nm.get_query_emb()
    gs, x = golden_inputs(qemb.shape[0])
    got, ref = corrections(gm, GossipBatch(gs, DEV, x=x), x, qemb, L)
    report(f"gossip_corr L={L}", got, ref)
    assert_logits_close(f"gossip correction L={L}", got, ref, tol=tol)


def test_deep_gossip_tail_in_row_chunks(nm, monkeypatch):
    """The post_mp tail of a depth-L pass runs in chunks of GOSSIP_DEEP_TAIL_ROWS rows: with chunks of 1000 rows (not
    a multiple of the query count) the result equals the one-chunk pass bit for bit and the oracle."""
    gm = gossip_model(3)
    qemb = nm.get_query_emb()
    gs, x = golden_inputs(qemb.shape[0])
    batch = GossipBatch(gs, DEV, x=x)
    gm.set_query_emb(qemb)
    with torch.no_grad():
        whole = gm.graph_to_count(batch).cpu()
    monkeypatch.setattr(GM, "GOSSIP_DEEP_TAIL_ROWS", 1000)
    with torch.no_grad():
        chunked = gm.graph_to_count(batch).cpu()
    same = torch.equal(chunked, whole)
    print(f"[chunks] {x.numel()} rows in chunks of 1000: equal to one chunk bit for bit: {same}")
    assert x.numel() > 3000 and same
    ref = OM.gossip_graph_to_count(cpu_sd(gm), x, batch.edge_index.numpy(), qemb.cpu(), layer_num=3) - x
    assert_logits_close("gossip correction L=3, chunked tail", chunked - x, ref, tol=2e-5)


def test_deep_gossip_syn_hub_shapes(nm):
    gm = gossip_model(3, gain=1.3)
    qemb = nm.get_query_emb()
    gs = syn_hub_graphs()
    deg = np.diff(GossipBatch(gs, DEV, x=torch.zeros(gs.num_nodes, 1)).rowptr.cpu().numpy())
    print(f"[shape] syn hub block: {gs.num_graphs} graphs, {gs.num_nodes} nodes, max degree {deg.max()}")
    g = torch.Generator().manual_seed(3)
    x = torch.rand(gs.num_nodes, qemb.shape[0], generator=g) * 25
    got, ref = corrections(gm, GossipBatch(gs, DEV, x=x), x, qemb, 3)
    report("syn gossip_corr L=3", got, ref)
    assert_logits_close("syn gossip correction L=3", got, ref)


def test_deep_gossip_more_than_64_queries():
    gm = gossip_model(3)
    g = torch.Generator().manual_seed(7)
    qemb = (torch.randn(70, 64, generator=g) * 0.5).to(DEV)
    gs, x = golden_inputs(70)
    got, ref = corrections(gm, GossipBatch(gs, DEV, x=x), x, qemb, 3)
    report("gossip_corr L=3 Q=70", got, ref)
    assert_logits_close("gossip correction L=3 Q=70", got, ref)


def test_gossip_layer_kernel_repeats_bit_for_bit():
    """The layer kernel on the hub shape, 20 launches: identical output and accumulator every time.  (Its values are
    checked per element against fp64 in tests/test_gossip_kernels_gpu.py::test_gossip_layer_against_fp64, this shape
    included.)"""
    gs = syn_hub_graphs()
    Q = 29
    batch = GossipBatch(gs, DEV, x=torch.zeros(gs.num_nodes, Q))
    N, R = gs.num_nodes, gs.num_nodes * Q
    g = torch.Generator().manual_seed(11)
    h = torch.rand(R, 64, generator=g).to(DEV)
    gate = torch.rand(Q, generator=g).to(DEV)
    c3 = torch.rand(R, 3, generator=g).to(DEV)
    v = (torch.randn(Q, 3, 64, generator=g) * 0.1).to(DEV)
    w = ops.split_f16_planes((torch.randn(64, 128, generator=g) * 0.05).to(DEV))
    p = ops.split_f16_planes((torch.randn(64, 64, generator=g) * 0.1).to(DEV))
    pn = ops.split_f16_planes((torch.randn(64, 64, generator=g) * 0.1).to(DEV))
    acc0 = torch.randn(R, 64, generator=g).to(DEV)
    outs, accs = [], []
    for _ in range(20):
        acc = acc0.clone()
        outs.append(ops.gossip_layer_f16(h, batch.rowptr, batch.col, N, Q, gate, c3, v, w, p, acc, pn=pn))
        accs.append(acc)
    torch.cuda.synchronize()
    same = all(torch.equal(o, outs[0]) for o in outs) and all(torch.equal(a, accs[0]) for a in accs)
    print(f"[repeat] gossip_layer_f16x3 x20 on {R} rows: bit-identical={same}")
    assert same


def test_pipeline_eager_and_replay_agree_at_depth_3(nm):
    from desco_amd.pipeline import InferencePipeline
    gm = gossip_model(3)
    gs = GraphSet.from_edge_lists(golden_graphs(max_n=60))
    pipe = InferencePipeline(nm, gm, gs, depth=4, device=DEV)
    eager = {k: v.clone() for k, v in pipe.run().items()}
    pipe.capture()
    rep = pipe.run_graph()
    torch.cuda.synchronize()
    same = all(torch.equal(eager[k], rep[k]) for k in ("node_count", "graph_gossip_count"))
    print(f"[replay] depth-3 pass: eager == captured replay bit for bit: {same}")
    assert same
    # and the pass against the oracle on its own inputs
    qemb = nm.get_query_emb()
    x = eager["x"].cpu()
    batch = GossipBatch(gs, DEV, x=x)
    ref = OM.gossip_graph_to_count(cpu_sd(gm), x, batch.edge_index.numpy(), qemb.cpu(), layer_num=3)
    report("pipeline node_count L=3", eager["node_count"], ref)
    assert_counts_close("pipeline node_count L=3", eager["node_count"].cpu(), ref)


# ---- training -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def train_setup(nm):
    graphs = golden_graphs(max_n=41)[:12]
    gs = GraphSet.from_edge_lists(graphs)
    g = torch.Generator().manual_seed(7)
    Q = nm.get_query_emb().shape[0]
    x = torch.rand(gs.num_nodes, Q, generator=g) * 20
    y = torch.floor(torch.rand(gs.num_nodes, Q, generator=g) * 25)
    return gs, x, y, nm.get_query_emb().detach()


def train_step(gm, gs, x, y, qemb, seed=None, step_no=0):
    if seed is not None:
        ops.manual_seed(seed, step=step_no)
    gm.set_query_emb(qemb)
    batch = GossipBatch(gs, DEV, x=x, y=y)
    gm.zero_grad()
    gm.train()
    loss = gm.train_forward(batch, 0)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), {n: p.grad.detach().clone() for n, p in gm.named_parameters() if p.grad is not None}, batch


def oracle_params(gm):
    """the model's parameters for the CPU oracle, in fp64: the gate gradients of these widened models are small
    residuals of large cancelling sums, and an fp64 reference keeps the oracle's own fp32 rounding out of the gap"""
    return {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in gm.state_dict().items()}


def check_grads(gm, grads, sd, what):
    worst = 0.0
    for name, _ in gm.named_parameters():
        ref = sd[name].grad
        if ref is None or float(ref.abs().max()) == 0.0:       # pre_mp (detached input) and anchor_mlp
            assert name not in grads or float(grads[name].abs().max()) == 0.0, name
            continue
        assert name in grads, name
        worst = max(worst, assert_grad_close(name, grads[name], ref.float(), tol=GOSSIP_GRAD_TOL))
    print(f"[parity] {what}: worst relative gradient error {worst:.3e}")


# (L = 1 at model seed 0 puts an activation of this batch within fp32 rounding of a ReLU / LeakyReLU kink: every layer-0
#  gradient then differs from the oracle's by the same 1e-3 .. 8e-3 whether or not the dropout path runs at p = 0, and
#  by 5e-7 with dropout 0.3 on the same weights; seed 2 is a point where the gradient is defined to fp32 accuracy.
#  tests/test_gossip_trunk_kernels_gpu.py holds the same nodes per element with relu' pinned to their own activations,
#  where no kink can hide or fake an error.)
@pytest.mark.parametrize("L,seed", [(1, 2), (3, 0)])
def test_deep_gossip_training_vs_oracle(train_setup, L, seed):
    gs, x, y, qemb = train_setup
    gm = gossip_model(L, seed=seed)
    loss, grads, batch = train_step(gm, gs, x, y, qemb)
    sd = oracle_params(gm)
    ref_loss = OM.gossip_loss(sd, x.double(), y.double(), batch.edge_index.numpy(), qemb.cpu().double(), layer_num=L)
    ref_loss.backward()
    report(f"gossip train loss L={L}", loss.reshape(1), ref_loss.detach().float().reshape(1))
    assert_loss_close(f"gossip train loss L={L}", loss, ref_loss.detach().float())
    check_grads(gm, grads, sd, f"gossip training L={L}")
    # the inference path equals the training path's forward in eval mode
    gm.eval()
    with torch.no_grad():
        pred = gm.graph_to_count(batch)
    pred_t = gm.emb_model(batch, query_emb=qemb)
    assert pred_t.requires_grad
    assert_logits_close(f"gossip inference path vs training path L={L}", pred, pred_t.detach())


@pytest.mark.parametrize("L", [1, 3])
def test_deep_gossip_training_with_dropout_vs_oracle(train_setup, L):
    """dropout 0.3 behind every layer and in post_mp.1: the factors the kernels used, exported per
    GossipTrunk.layer_site(l) and SITE_POST, fed to the oracle."""
    gs, x, y, qemb = train_setup
    p, seed = 0.3, 4242
    gm = gossip_model(L, dropout=p)
    loss, grads, batch = train_step(gm, gs, x, y, qemb, seed=seed, step_no=3)
    N, Q = x.shape
    key = torch.tensor([seed, 3], dtype=torch.int64, device=DEV)
    T = AG.GossipTrunk
    lm = [ops.dropout_mask(ops.DropSite(key, T.layer_site(l), p), N * Q, 64).cpu().view(N, Q, 64)
          for l in range(1, L + 1)]
    pm = ops.dropout_mask(ops.DropSite(key, T.SITE_POST, p), N * Q, 64).cpu().view(N, Q, 64)
    print(f"[dropout] L={L} sites {[T.layer_site(l) for l in range(1, L + 1)]} + {T.SITE_POST}: dropped fractions "
          f"{[round(float((m == 0).double().mean()), 3) for m in lm + [pm]]}")
    sd = oracle_params(gm)
    ref_loss = OM.gossip_loss(sd, x.double(), y.double(), batch.edge_index.numpy(), qemb.cpu().double(), layer_num=L,
                              masks=([m.double() for m in lm], pm.double()))
    ref_loss.backward()
    assert_loss_close(f"gossip train loss L={L}, dropout {p}", loss, ref_loss.detach().float())
    plain = OM.gossip_loss({k: v.detach() for k, v in sd.items()}, x.double(), y.double(), batch.edge_index.numpy(),
                           qemb.cpu().double(), layer_num=L)
    assert abs(float(plain) - float(ref_loss.detach())) / abs(float(ref_loss.detach())) > 1e-4
    check_grads(gm, grads, sd, f"gossip training L={L}, dropout {p}")


def test_deep_gossip_trainer_capture_equals_eager(tmp_path, train_setup):
    """Trainer(graph_capture=True) at L = 3 with dropout 0.01: the replayed steps give the eager run's validation
    losses and weights bit for bit."""
    from desco_amd.trainer import Trainer
    gs, x, y, qemb = train_setup

    class DM:
        def __init__(self):
            self.b = [GossipBatch(gs, DEV, x=x, y=y)]

        def train_dataloader(self):
            return self.b

        def val_dataloader(self):
            return self.b

    outs = []
    for capture in (False, True):
        gm = gossip_model(3, dropout=0.01)
        gm.set_query_emb(qemb)
        ops.manual_seed(99)
        tr = Trainer(max_epochs=4, default_root_dir=str(tmp_path / f"c{int(capture)}"), graph_capture=capture)
        tr.fit(gm, DM())
        torch.cuda.synchronize()
        outs.append(({k: v.detach().clone() for k, v in gm.state_dict().items()},
                     [h["gossip_counting_val_loss"] for h in tr.history]))
    (sa, ha), (sb, hb) = outs
    print(f"[trainer] L=3 eager val losses {ha}; replayed {hb}")
    assert ha == hb
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_main_trains_and_predicts_at_gossip_depth_3(tmp_path):
    """main.py end to end on toy TU data with --gossip_layer_num 3 (as tests/test_main_gpu.py at the default depth):
    train both stages, reload last.ckpt, predict, write the artefacts; the gossip checkpoint carries convs.2.*."""
    import argparse
    import main as driver
    from desco_amd import config
    from desco_amd.ckpt import load_checkpoint
    from desco_amd.data import STANDARD_QUERY_IDS
    from test_main_gpu import _write_tu
    root = str(tmp_path / "data")
    _write_tu(root, "TOY", golden_graphs(max_n=30))
    p = argparse.ArgumentParser()
    config.parse_optimizer(p)
    config.parse_neighborhood(p)
    config.parse_gossip(p)
    args = p.parse_args(["--train_dataset", "TOY_train", "--valid_dataset", "TOY_val", "--test_dataset",
                         "TOY_test", "--neigh_epoch_num", "1", "--gossip_epoch_num", "2", "--gossip_layer_num", "3",
                         "--neigh_batch_size", "64", "--gossip_batch_size", "4",
                         "--neigh_model_path", str(tmp_path / "ckpt_n"), "--gossip_model_path",
                         str(tmp_path / "ckpt_g"), "--train_neigh", "--train_gossip", "--test_gossip",
                         "--output_dir", str(tmp_path / "out")])
    an, ag, ao = config.split_namespaces(args)
    rep = driver.main(an, ag, ao, train_neighborhood=True, train_gossip=True, test_gossip=True,
                      atlas_query_ids=STANDARD_QUERY_IDS, output_dir=str(tmp_path / "out"), data_root=root)
    assert all(np.isfinite(rep["graphlet_mae_gossip"]))
    for f in ["gossip_graphlet_TOY_test.csv", "gossip_gate_TOY_test.csv", "gossip_node_TOY_test_results.csv",
              "graphlet_count_TOY_test.csv", "analyze_results_TOY_test.txt"]:
        assert (tmp_path / "out" / f).exists(), f
    ck = tmp_path / "ckpt_g" / "last.ckpt"
    keys = list(load_checkpoint(str(ck))["state_dict"])
    conv2 = [k for k in keys if ".convs.2." in k]
    print(f"[main] gossip checkpoint: {len(keys)} tensors, {len(conv2)} of convs.2")
    assert conv2 and not any(".convs.3." in k for k in keys)
    rep2 = driver.main(an, ag, ao, train_neighborhood=False, train_gossip=False, test_gossip=True,
                       neighborhood_checkpoint=str(tmp_path / "ckpt_n" / "last.ckpt"), gossip_checkpoint=str(ck),
                       atlas_query_ids=STANDARD_QUERY_IDS, output_dir=str(tmp_path / "out2"), data_root=root)
    assert all(np.isfinite(rep2["graphlet_mae_gossip"]))
    assert (tmp_path / "out2" / "gossip_node_TOY_test_results.csv").exists()
