"""The plain GIN / GCN models (--neigh_conv_type GIN / GCN: a homogeneous NeighborhoodCountingModel on the fused
plain-layer kernel, gnn_model.plain_forward) on the GPU, over the golden graphs' restricted partition with the 0/1 anchor
feature: inference against the CPU restatement (tests/plain_reference.py), fused against un-fused (PLAIN_FUSED), the eps
buffer, one training step against autograd through the restatement (dropout 0 and with the kernels' masks), the
checkpoint round trip, the refusals, the driver and the inference pipeline.  The suite's one float gate (helpers)."""
import os
import re
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import homo_reference as HR
import plain_reference as PR
from desco_amd import gnn_model as GM
from desco_amd import ops
from desco_amd.batch import NeighborhoodBatch
from desco_amd.graphs import GraphSet
from desco_amd.lightning_model import NeighborhoodCountingModel
from desco_amd.partition import build_partition, build_partition_device
from oracle import model as OM

from helpers import (GRAD_TOL, LOGIT_TOL, LOSS_TOL, assert_counts_close, assert_grad_close, assert_logits_close, assert_loss_close, cpu_sd,
                     golden_graphs, log_space_err, standard_queries)
from test_homo_reference_host import FIVE_CYCLE
from test_plain_reference_host import plain_model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH = 4

# Weight gains, chosen from the REFERENCE's own error (the float32 restatement against its float64 evaluation, in the
# gate's metric, on this partition; measured on the CPU with the model classes' own seeded init and 0.1 bias noise):
#   GIN  gain 1.0: 1.9e-6 / 2.6e-6 (2 layers, widths 64 / 100), 3.6e-6 / 5.4e-6 (8 layers); embedding std 0.21 - 0.52;
#        with eps = 0.25: 2.7e-6 / 2.4e-6 and 5.4e-6 / 5.7e-6, std 0.22 - 0.61
#   GCN  GCNConv initialises with glorot, whose bound is sqrt(3) times the default nn.Linear's: at gain 1.0 two layers
#        sit at 5.0e-6 / 9.3e-6 (no room under LOGIT_TOL / 5), at 0.6 eight layers reach 1e-4 - 2e-4.  Gain 0.8 for two
#        layers: 2.0e-6 / 3.0e-6, std 0.27 / 0.75; gain 0.37 for eight: 3.3e-6 / 2.9e-6, std 0.28 / 0.22 (at 0.4 the own
#        error is 4.8e-6 / 7.5e-6 with one BLAS and 8.4e-6 / 9.0e-6 with another; at 0.35 the spread falls to 0.15 / 0.11,
#        at 0.3 to 0.02).
GAIN = {("GIN", 2): 1.0, ("GIN", 8): 1.0, ("GCN", 2): 0.8, ("GCN", 8): 0.37}


def on_gpu(nm):
    nm = nm.to(DEV)
    nm.set_queries(standard_queries()[0], hetero=False)
    return nm


@pytest.fixture(scope="module")
def golden_case():
    """the golden graphs' restricted partition (built on the device), the restatement's batches over the same
    neighborhoods; shared and left unchanged"""
    graphs = golden_graphs()
    _, queries = standard_queries()
    part = build_partition_device(GraphSet.from_edge_lists(graphs), DEPTH, DEV, restricted=True)
    neighs = HR.restricted_neighborhoods(graphs, DEPTH)
    assert part.neigh_index.tolist() == [[g, v] for g, v, _, _ in neighs]
    assert (part.num_neigh, part.num_rows) == (637, 10868)
    return {"part": part, "hb": HR.homo_batch([(n, e) for _, _, n, e in neighs]), "qb": HR.homo_query_batch(queries),
            "queries": queries}


def own_error(sd, hb, layer_num, conv, ref_emb):
    """the float32 restatement against its float64 evaluation, in the gate's metric"""
    torch.set_default_dtype(torch.float64)
    try:
        e64 = PR.base_gnn_plain({k: v.double() for k, v in sd.items()}, "emb_model",
                                dict(hb, node_feature=hb["node_feature"].double()), layer_num, conv)
    finally:
        torch.set_default_dtype(torch.float32)
    return log_space_err(ref_emb, e64)


def _check_inference(golden_case, conv, layer_num, hidden, eps, monkeypatch):
    part, hb, qb = golden_case["part"], golden_case["hb"], golden_case["qb"]
    nm = on_gpu(plain_model(conv, layer_num, hidden, gain=GAIN[conv, layer_num], eps=eps))
    assert nm.emb_model.gnn_core.node_types is None and nm.emb_model.is_wide() and nm.emb_model.gnn_core.is_plain()
    sd = cpu_sd(nm)
    ref_emb, ref_logits = PR.plain_logits(sd, hb, qb, layer_num, conv)
    ref_q = PR.base_gnn_plain(sd, "emb_model_query", qb, layer_num, conv)
    name = f"{conv} L={layer_num} h={hidden}" + (f" eps={eps}" if eps else "")
    own = own_error(sd, hb, layer_num, conv, ref_emb)
    spread = float(ref_emb.std(0).mean())
    print(f"[reference] {name}: float32 restatement against its float64 evaluation {own:.2e}, embedding std {spread:.3f}")
    assert own <= LOGIT_TOL / 5, f"{name}: the reference's own error {own:.2e} leaves the gate no room"
    assert spread > 0.1, "embeddings do not depend on the neighborhood"
    batch = NeighborhoodBatch(part, DEV, anchor_flag=True)
    results = {}
    for fused in (True, False):
        monkeypatch.setattr(GM, "PLAIN_FUSED", fused)
        nm.invalidate_caches()
        tag = name + (" fused" if fused else " un-fused")
        with torch.no_grad():
            emb = nm.graph_to_embed(batch)
            logits = nm._logits(batch, exp2=False)
            counts = nm.graph_to_count(batch)
            qemb = nm.get_query_emb()
        assert logits.shape == (part.num_neigh, len(golden_case["queries"])) and emb.shape == (part.num_neigh, hidden)
        assert_logits_close(tag + " target embeddings", emb, ref_emb)
        assert_logits_close(tag + " query embeddings", qemb, ref_q)
        assert_logits_close(tag + " head logits", logits, ref_logits)
        assert_counts_close(tag + " counts", counts, OM.count_from_logits(ref_logits))
        results[fused] = (emb.clone(), logits.clone())
    # the two forms do not coincide by construction (16-wide K steps on 32x32x16 MFMAs in gemm_f16x3, 32-wide steps on
    # 16x16x32 in the fused kernel): held to each other within the gate, not bit for bit
    assert_logits_close(name + " fused against un-fused embeddings", results[True][0], results[False][0].cpu())
    assert_logits_close(name + " fused against un-fused logits", results[True][1], results[False][1].cpu())
    return nm, batch


# ---- 1. inference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer_num,hidden", [(2, 64), (8, 64), (2, 100), (8, 100)])
@pytest.mark.parametrize("conv", PR.CONVS)
def test_logits_match_the_restatement_fused_and_unfused(golden_case, monkeypatch, conv, layer_num, hidden):
    """Embeddings (target and query), logits and counts within LOGIT_TOL of tests/plain_reference.py, with the fused
    plain-layer kernel and with the un-fused composition; each case first asserts the reference's own condition (its
    float32 evaluation within LOGIT_TOL / 5 of its float64 one, embedding std above 0.1: GAIN above)."""
    nm, _ = _check_inference(golden_case, conv, layer_num, hidden, None, monkeypatch)
    # a batch without the anchor feature is refused, not silently run as all-count rows
    with pytest.raises(ValueError, match="node_feature"):
        nm.graph_to_embed(NeighborhoodBatch(golden_case["part"], DEV))


@pytest.mark.parametrize("layer_num,hidden", [(2, 64), (8, 100)])
def test_gin_with_eps_a_quarter_matches_the_restatement(golden_case, monkeypatch, layer_num, hidden):
    """the eps buffers set to 0.25 (a hand-edited checkpoint): z = agg + 1 + eps x, the kernel's self_scale"""
    nm, batch = _check_inference(golden_case, "GIN", layer_num, hidden, 0.25, monkeypatch)
    monkeypatch.setattr(GM, "PLAIN_FUSED", True)
    with torch.no_grad():
        with_eps = nm.graph_to_embed(batch).clone()
        for m in (nm.emb_model, nm.emb_model_query):
            for e in m.gnn_core.eps:
                e.eps.zero_()                       # in place, on the device: read by the next launch without a re-pack
        assert log_space_err(nm.graph_to_embed(batch), with_eps) > 10 * LOGIT_TOL


def test_core_forward_on_plain_tensors_runs_the_gin_and_gcn_branches(golden_case):
    """BaseGNNCore.forward(x, edge_index) of a plain core: op by op, against the restatement's layer loop"""
    hb = golden_case["hb"]
    rows = slice(0, 400)
    keep = (hb["edge_index"] < 400).all(0)
    sub = {"node_feature": hb["node_feature"][rows], "edge_index": hb["edge_index"][:, keep]}
    for conv, hidden, eps in (("GIN", 64, 0.25), ("GCN", 100, None)):
        nm = on_gpu(plain_model(conv, 2, hidden, gain=GAIN[conv, 2], eps=eps))
        got = nm.emb_model.gnn_core(sub["node_feature"].to(DEV), sub["edge_index"].to(DEV))
        want = torch.cat(PR.plain_layers(cpu_sd(nm), "emb_model", sub, 2, conv), 1)
        assert got.shape == (400, 3 * hidden)
        assert_logits_close(f"{conv} core forward", got, want)


# ---- 2. one training step -------------------------------------------------------------------------------------------
def train_case():
    graphs = [FIVE_CYCLE] + golden_graphs(max_n=20)[:3]
    neighs = HR.restricted_neighborhoods(graphs, DEPTH)
    part = build_partition(GraphSet.from_edge_lists(graphs), DEPTH, restricted=True)
    assert part.neigh_index.tolist() == [[g, v] for g, v, _, _ in neighs] and 16 < part.num_neigh <= 64
    _, queries = standard_queries()
    g = torch.Generator().manual_seed(9)
    y = torch.floor(torch.rand(part.num_neigh, len(queries), generator=g) ** 3 * 40)
    return part, HR.homo_batch([(n, e) for _, _, n, e in neighs]), HR.homo_query_batch(queries), queries, y


@pytest.mark.parametrize("hidden", [64, 100])
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("conv", PR.CONVS)
def test_training_step_matches_autograd_through_the_restatement(conv, p, hidden):
    """Loss within LOSS_TOL and every parameter's gradient within GRAD_TOL of torch autograd through plain_reference, at
    dropout 0 and with the kernels' own masks injected (query model: the first key drawn, target model: the second; site
    2 l for all rows of layer l, POST_DROP_SITE for post_mp.1).  The gradients have the parameters' true shapes (the padded
    channels get none) and eps, a buffer, gets none."""
    L = 2
    part, hb, qb, queries, y = train_case()
    nm = on_gpu(plain_model(conv, L, hidden, dropout=p, gain=GAIN[conv, L], eps=0.25 if conv == "GIN" else None))
    batch = NeighborhoodBatch(part, DEV, y=y, anchor_flag=True)
    seed = 777
    ops.manual_seed(seed, step=5)
    nm.train()
    nm.zero_grad()
    loss = nm.train_forward(batch, 0)
    loss.backward()
    torch.cuda.synchronize()
    masks_t = masks_q = None
    if p > 0.0:
        assert ops.rng_state(DEV).cpu().tolist() == [seed, 7]
        kq = torch.tensor([seed, 5], dtype=torch.int64, device=DEV)
        kt = torch.tensor([seed, 6], dtype=torch.int64, device=DEV)
        B, N, nq = part.num_neigh, part.num_rows, sum(n for n, _ in queries)
        wp = GM.padded_width(hidden)
        rows = torch.from_numpy(HR.partition_rows(part))

        def fac(key, site, r):
            return ops.dropout_mask(ops.DropSite(key, site, p), r, wp).cpu()[:, :hidden]

        def layer_mask(l):
            m = fac(kt, GM.wide_layer_drop_site(l), N)
            out = torch.empty_like(m)
            out[rows] = m                       # the kernels' row layout -> the restatement's
            return out
        masks_t = ([layer_mask(l) for l in range(L)], fac(kt, GM.POST_DROP_SITE, B))
        masks_q = ([fac(kq, GM.wide_layer_drop_site(l), nq) for l in range(L)], fac(kq, GM.POST_DROP_SITE, len(queries)))
    sd = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point() and not k.endswith(".eps"))
          for k, v in nm.state_dict().items()}
    ref_loss = OM.train_loss_from_logits(PR.plain_logits(sd, hb, qb, L, conv, masks_t, masks_q)[1], y)
    ref_loss.backward()
    name = f"{conv} train step, h={hidden}, dropout {p}"
    assert_loss_close(name + " loss", loss.detach(), ref_loss.detach())
    if p > 0.0:
        plain = OM.train_loss_from_logits(PR.plain_logits({k: v.detach() for k, v in sd.items()}, hb, qb, L, conv)[1], y)
        # the masks matter: a step that ignored them would miss the loss gate (measured 5e-4 .. 1e-2 relative)
        assert abs(float(plain) - float(ref_loss.detach())) / abs(float(ref_loss.detach())) > 2 * LOSS_TOL
    worst, checked = 0.0, 0
    for pname, prm in nm.named_parameters():
        assert not pname.endswith(".eps")
        ref = sd[pname].grad
        if ref is None or float(ref.abs().max()) == 0.0:          # (the query model's anchor_mlp: never applied)
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, pname
            continue
        assert prm.grad is not None and prm.grad.shape == prm.shape, pname
        worst = max(worst, assert_grad_close(pname, prm.grad, ref, tol=GRAD_TOL))
        checked += 1
    print(f"[parity] {name}: worst relative gradient error over {checked} tensors: {worst:.3e}")
    assert checked >= 2 * (2 + (4 if conv == "GIN" else 2) * L + 8) + 2      # both models' core + post_mp, anchor, head
    for m in (nm.emb_model, nm.emb_model_query):
        for e in getattr(m.gnn_core, "eps", []):
            assert not e.eps.requires_grad and e.eps.grad is None and float(e.eps) == 0.25


# ---- 3. checkpoint, refusals ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("conv", PR.CONVS)
def test_a_reference_shaped_checkpoint_loads_and_predicts_the_same_counts(golden_case, tmp_path, conv):
    """a Lightning-shaped file holding the reference's key names (gnn_core.updates.l.{0,2}.*, gnn_core.eps.l.eps / gnn_core
    .convs.l.lin.weight, gnn_core.convs.l.bias) and hyper-parameters loads, and predicts bit-identical counts"""
    L = 2
    nm = on_gpu(plain_model(conv, L, 64, gain=GAIN[conv, L], eps=0.25 if conv == "GIN" else None))
    batch = NeighborhoodBatch(golden_case["part"], DEV, anchor_flag=True)
    counts = nm.graph_to_count(batch).clone()
    sd = cpu_sd(nm)
    core = [k.split("gnn_core.")[1] for k in sd if k.startswith("emb_model.gnn_core.")]
    want = ["pre_mp.0.weight", "pre_mp.0.bias"]
    for l in range(L):
        want += [f"updates.{l}.0.weight", f"updates.{l}.0.bias", f"updates.{l}.2.weight", f"updates.{l}.2.bias"] \
            if conv == "GIN" else [f"convs.{l}.lin.weight", f"convs.{l}.bias"]
    if conv == "GIN":
        want += [f"eps.{l}.eps" for l in range(L)]
    assert sorted(core) == sorted(want)
    path = str(tmp_path / f"{conv}.ckpt")
    torch.save({"state_dict": sd, "hyper_parameters": {"input_dim": 1, "hidden_dim": 64, "args": nm.args}}, path)
    back = on_gpu(NeighborhoodCountingModel.load_from_checkpoint(path))
    assert back.emb_model.gnn_core.conv_type == conv and back.emb_model.gnn_core.is_plain()
    assert torch.equal(back.graph_to_count(batch), counts)
    again = str(tmp_path / f"{conv}_again.ckpt")
    back.save_checkpoint(again)
    third = on_gpu(NeighborhoodCountingModel.load_from_checkpoint(again))
    assert torch.equal(third.graph_to_count(batch), counts)


@pytest.mark.parametrize("conv,hidden", [("GIN", 64), ("GCN", 100)])
def test_graph_capture_is_refused_for_a_plain_model(tmp_path, conv, hidden):
    """by a message naming --neigh_conv_type, ahead of the width check (hidden 100) and the homogeneous one"""
    from desco_amd.trainer import Trainer
    nm = on_gpu(plain_model(conv, 2, hidden))
    with pytest.raises(NotImplementedError, match=f"--neigh_conv_type {conv}"):
        Trainer(max_epochs=1, devices=[0], default_root_dir=str(tmp_path), graph_capture=True).fit(nm, datamodule=None)


# ---- 4. the driver and the inference pipeline -----------------------------------------------------------------------
def test_driver_trains_a_gin_model_and_the_pipeline_agrees(tmp_path):
    """``ablation_gnns.py --neigh_conv_type GIN`` in a fresh process: one epoch, two layers, on the MUTAG-shaped synthetic
    split; then InferencePipeline(nm, None, graphs) on the driver's best checkpoint against the driver's own prediction."""
    from desco_amd.data import load_data
    from desco_amd.pipeline import InferencePipeline
    out, ckpt, data = tmp_path / "out", tmp_path / "ckpt", tmp_path / "data"
    cmd = [sys.executable, os.path.join(ROOT, "ablation_gnns.py"), "--data_root", str(data),
           "--train_dataset", "MUTAG_train", "--valid_dataset", "MUTAG_val", "--test_dataset", "MUTAG_test",
           "--neigh_epoch_num", "1", "--neigh_layer_num", "2", "--neigh_batch_size", "64", "--neigh_model_path", str(ckpt),
           "--neigh_conv_type", "GIN", "--train_neigh", "--output_dir", str(out), "--seed", "0", "--gpu", "0"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    print(p.stdout[-1500:])
    cfg = (out / "config_MUTAG_test.txt").read_text()
    assert "use_hetero=False" in cfg and "use_tconv=False" in cfg and "conv_type='GIN'" in cfg and "layer_num=2" in cfg
    best = re.search(r"best neighborhood model path:\s+(\S+)", p.stdout).group(1)
    assert os.path.exists(best) and (ckpt / "last.ckpt").exists()
    back = NeighborhoodCountingModel.load_from_checkpoint(best)
    assert back.emb_model.gnn_core.is_plain() and back.args.conv_type == "GIN" and back.args.use_hetero is False
    keys = back.state_dict()
    assert "emb_model.gnn_core.updates.1.2.weight" in keys and "emb_model.gnn_core.eps.1.eps" in keys
    assert not any(".gnn_core.convs." in k for k in keys)
    val = float(re.search(r"final neighborhood_counting_val_loss: (\S+)", p.stdout).group(1))
    test = float(re.search(r"'test_loss': ([0-9.eE+-]+)", p.stdout).group(1))
    assert np.isfinite(val) and np.isfinite(test)
    driver_pred = pd.read_csv(out / "neighborhood_node_MUTAG_test_results.csv", index_col=0).to_numpy(dtype=np.float32)
    assert np.isfinite(driver_pred).all()
    back = back.to(DEV)
    back.set_queries(standard_queries()[0], hetero=False)
    graphs = load_data("MUTAG_test", root_folder=str(data))
    pipe = InferencePipeline(back, None, graphs, depth=4, device=DEV)
    assert pipe.partition_backend == "device" and pipe.restricted and pipe.partition.restricted
    res = pipe.run(gossip=False)
    assert set(res) == {"neigh_count", "graph_neigh_count"}
    assert res["neigh_count"].shape == driver_pred.shape
    assert_counts_close("pipeline against the driver's prediction", res["neigh_count"], torch.from_numpy(driver_pred))
