"""The homogeneous ablation (ablation_gnns.py) on the GPU: a NeighborhoodCountingModel built with use_hetero=False -- one
pre_mp / convs[l].lin / updates[l] read by every row type and relation slot of the fused kernels -- over the restricted
neighborhoods with the 0/1 anchor feature: inference against the CPU restatement (tests/homo_reference.py) and against the
untied hetero twin, one training step against autograd through the restatement (dropout 0 and with the kernels' masks),
the shared parameters' gradients against the sum over the twin's copies, the graph-capture refusal, the driver and the
inference pipeline."""
import argparse
import os
import re
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import homo_reference as HR
from desco_amd import gnn_model as GM
from desco_amd import ops
from desco_amd.batch import NeighborhoodBatch
from desco_amd.graphs import GraphSet
from desco_amd.lightning_model import NeighborhoodCountingModel
from desco_amd.partition import build_partition, build_partition_device
from oracle import model as OM

from helpers import (GRAD_TOL, LOGIT_TOL, assert_counts_close, assert_grad_close, assert_logits_close, assert_loss_close, cpu_sd,
                     golden_graphs, log_space_err, neigh_args, standard_queries)
from test_homo_reference_host import FIVE_CYCLE, homo_model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH = 4


def on_gpu(nm):
    nm = nm.to(DEV)
    nm.set_queries(standard_queries()[0], hetero=False)
    return nm


def hetero_twin(nm, layer_num, hidden, dropout=0.0):
    """the hetero use_tconv=False model whose per-type / per-relation weights are copies of ``nm``'s shared ones
    (homo_reference.tied_hetero_state_dict: the count destinations' second relation carries a zero bias)"""
    tw = NeighborhoodCountingModel(1, hidden, neigh_args(layer_num=layer_num, hidden_dim=hidden, use_tconv=False,
                                                         dropout=dropout)).to_hetero_old(False, False)
    tw.load_state_dict(HR.tied_hetero_state_dict(cpu_sd(nm), layer_num))
    tw = tw.to(DEV)
    tw.set_queries(standard_queries()[0])
    return tw


@pytest.fixture(scope="module")
def golden_case():
    """the golden graphs' restricted partition (built on the device), the restatement's batches over the same
    neighborhoods; shared and left unchanged"""
    graphs = golden_graphs()
    _, queries = standard_queries()
    part = build_partition_device(GraphSet.from_edge_lists(graphs), DEPTH, DEV, restricted=True)
    neighs = HR.restricted_neighborhoods(graphs, DEPTH)
    assert part.neigh_index.tolist() == [[g, v] for g, v, _, _ in neighs]
    return {"part": part, "hb": HR.homo_batch([(n, e) for _, _, n, e in neighs]), "qb": HR.homo_query_batch(queries),
            "queries": queries}


def own_error(sd, hb, qb, layer_num, ref_emb):
    """the float32 restatement against its float64 evaluation, in the gate's metric"""
    torch.set_default_dtype(torch.float64)
    try:
        e64 = HR.base_gnn_homo({k: v.double() for k, v in sd.items()}, "emb_model",
                               dict(hb, node_feature=hb["node_feature"].double()), layer_num)
    finally:
        torch.set_default_dtype(torch.float32)
    return log_space_err(ref_emb, e64)


# ---- 1. inference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer_num,hidden", [(2, 64), (8, 64), (2, 100), (8, 100)])
def test_logits_match_the_restatement_and_the_untied_twin(golden_case, layer_num, hidden):
    """Embeddings and logits within LOGIT_TOL of tests/homo_reference.py, and bit-identical to the hetero use_tconv=False
    twin on the same partition and the same 0/1 feature: both forms fold the same operands ((U_n W)^T per slot, U_x^T,
    U_n b + c -- the twin's second bias is zero, and b + 0 == b).

    The weight gain is chosen from the REFERENCE's own error: the float32 restatement against its float64 evaluation
    sits at 4.8e-6 / 8.0e-6 (2 layers, gain 1.3, widths 64 / 100) and 4.5e-6 / 5.4e-6 (8 layers, gain 1.0) in the gate's
    metric (at gain 1.3 eight layers reach 3.5e-4, seven times the gate); the test asserts it stays under a fifth of
    the gate."""
    part, hb, qb = golden_case["part"], golden_case["hb"], golden_case["qb"]
    nm = on_gpu(homo_model(layer_num, hidden, gain=1.3 if layer_num == 2 else 1.0))
    assert nm.emb_model.gnn_core.node_types is None and nm.emb_model.is_wide() == (hidden != 64)
    sd = cpu_sd(nm)
    ref_emb, ref_logits = HR.homo_logits(sd, hb, qb, layer_num)
    name = f"homogeneous L={layer_num} h={hidden}"
    own = own_error(sd, hb, qb, layer_num, ref_emb)
    print(f"[reference] {name}: float32 restatement against its float64 evaluation {own:.2e}")
    assert own <= LOGIT_TOL / 5, f"{name}: the reference's own error {own:.2e} leaves the gate no room"
    assert float(ref_emb.std(0).mean()) > 0.1, "embeddings do not depend on the neighborhood"
    batch = NeighborhoodBatch(part, DEV, anchor_flag=True)
    with torch.no_grad():
        emb = nm.graph_to_embed(batch)
        logits = nm._logits(batch, exp2=False)
        counts = nm.graph_to_count(batch)
    assert logits.shape == (part.num_neigh, len(golden_case["queries"]))
    assert_logits_close(name + " target embeddings", emb, ref_emb)
    assert_logits_close(name + " head logits", logits, ref_logits)
    assert_counts_close(name + " counts", counts, OM.count_from_logits(ref_logits))
    # the untied twin, fed the same feature as a plain per-row tensor (the --use_node_feature path)
    tw = hetero_twin(nm, layer_num, hidden)
    tb = NeighborhoodBatch(part, DEV, node_feature=batch.node_feature.clone())
    with torch.no_grad():
        assert torch.equal(tw.get_query_emb(), nm.get_query_emb())
        assert torch.equal(tw.graph_to_embed(tb), emb)
        assert torch.equal(tw._logits(tb, exp2=False), logits)
    # a batch without the anchor feature is refused, not silently run as all-count rows
    with pytest.raises(ValueError, match="node_feature"):
        nm.graph_to_embed(NeighborhoodBatch(part, DEV))


def test_core_forward_on_plain_tensors_runs_the_sage_branch(golden_case):
    """BaseGNNCore.forward(x, edge_index) of a homogeneous core: op by op, against the restatement's layer loop"""
    hb = golden_case["hb"]
    nm = on_gpu(homo_model(2, 64))
    rows = slice(0, 400)
    keep = (hb["edge_index"] < 400).all(0)
    x, ei = hb["node_feature"][rows], hb["edge_index"][:, keep]
    got = nm.emb_model.gnn_core(x.to(DEV), ei.to(DEV))
    sd = cpu_sd(nm)
    h = torch.nn.functional.linear(x, sd["emb_model.gnn_core.pre_mp.0.weight"], sd["emb_model.gnn_core.pre_mp.0.bias"])
    want = [h]
    for l in range(2):
        agg = torch.zeros_like(h).index_add_(0, ei[1], h[ei[0]])
        xn = torch.nn.functional.linear(agg, sd[f"emb_model.gnn_core.convs.{l}.lin.weight"],
                                        sd[f"emb_model.gnn_core.convs.{l}.lin.bias"])
        h = torch.relu(torch.nn.functional.linear(torch.cat((xn, h), 1), sd[f"emb_model.gnn_core.updates.{l}.weight"],
                                                  sd[f"emb_model.gnn_core.updates.{l}.bias"]))
        want.append(h)
    assert got.shape == (400, 192)
    assert_logits_close("homogeneous core forward", got, torch.cat(want, 1))


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
def test_training_step_matches_autograd_through_the_restatement(p, hidden):
    """Loss within LOSS_TOL and every parameter's gradient within GRAD_TOL of torch autograd through homo_reference, at
    dropout 0 and with the kernels' own masks injected (query model: the first key drawn, target model: the second;
    width 64: sites 2 l for count rows, 2 l + 1 for canonical rows; wide path: site 2 l for all rows; post_mp.1)."""
    L = 2
    part, hb, qb, queries, y = train_case()
    nm = on_gpu(homo_model(L, hidden, dropout=p))
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
        Nc, B, N, nq = part.num_count, part.num_neigh, part.num_rows, sum(n for n, _ in queries)
        wp = GM.padded_width(hidden)
        rows = torch.from_numpy(HR.partition_rows(part))

        def fac(key, site, r):
            return ops.dropout_mask(ops.DropSite(key, site, p), r, wp).cpu()[:, :hidden]

        def layer_mask(l):
            if hidden == 64:
                m = torch.cat([fac(kt, 2 * l, Nc), fac(kt, 2 * l + 1, B)])
            else:
                m = fac(kt, GM.wide_layer_drop_site(l), N)
            out = torch.empty_like(m)
            out[rows] = m                       # the kernels' row layout -> the restatement's
            return out
        masks_t = ([layer_mask(l) for l in range(L)], fac(kt, GM.POST_DROP_SITE, B))
        masks_q = ([fac(kq, 2 * l, nq) for l in range(L)], fac(kq, GM.POST_DROP_SITE, len(queries)))
    sd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in nm.state_dict().items()}
    ref_loss = OM.train_loss_from_logits(HR.homo_logits(sd, hb, qb, L, masks_t, masks_q)[1], y)
    ref_loss.backward()
    name = f"homogeneous train step, h={hidden}, dropout {p}"
    assert_loss_close(name + " loss", loss.detach(), ref_loss.detach())
    if p > 0.0:
        plain = OM.train_loss_from_logits(HR.homo_logits({k: v.detach() for k, v in sd.items()}, hb, qb, L)[1], y)
        assert abs(float(plain) - float(ref_loss.detach())) / abs(float(ref_loss.detach())) > 1e-3     # the masks matter
    worst, checked = 0.0, 0
    for pname, prm in nm.named_parameters():
        ref = sd[pname].grad
        if ref is None or float(ref.abs().max()) == 0.0:          # (the query model's anchor_mlp: never applied)
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, pname
            continue
        assert prm.grad is not None, pname
        worst = max(worst, assert_grad_close(pname, prm.grad, ref, tol=GRAD_TOL))
        checked += 1
    print(f"[parity] {name}: worst relative gradient error over {checked} tensors: {worst:.3e}")
    assert checked >= 2 * (2 + 4 * L + 8) + 2                      # both models' core + post_mp, anchor, head


@pytest.mark.parametrize("hidden", [64, 100])
def test_shared_gradients_are_the_sums_over_the_untied_twin(hidden):
    """One step of the homogeneous model and one of its untied twin on the same batch: every shared parameter's gradient
    is the sum of the gradients of its copies (count + canonical for pre_mp / updates; the three relations for a conv
    weight; for a conv bias the two relations that carry it -- the twin's zero bias is not a use of the shared one)."""
    L = 2
    part, _, _, _, y = train_case()
    nm = on_gpu(homo_model(L, hidden))
    tw = hetero_twin(nm, L, hidden)
    for m, b in ((nm, NeighborhoodBatch(part, DEV, y=y, anchor_flag=True)),
                 (tw, NeighborhoodBatch(part, DEV, y=y, node_feature=torch.cat([torch.zeros(part.num_count, 1),
                                                                                torch.ones(part.num_neigh, 1)])))):
        m.train()
        m.zero_grad()
        m.train_forward(b, 0).backward()
    torch.cuda.synchronize()
    tg = {k: v.grad for k, v in tw.named_parameters()}
    checked = 0
    for name, prm in nm.named_parameters():
        if ".gnn_core." not in name:
            copies = [name]
        else:
            copies = [k for k, v in HR.tied_hetero_state_dict({name: prm.detach()}, L).items()
                      if not (k.endswith("canonical__union__count.lin.bias"))]
        grads = [tg[k] for k in copies if tg[k] is not None]
        if not grads:
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, name
            continue
        assert_grad_close(name + " (sum over the twin's copies)", prm.grad, torch.stack(grads).sum(0).cpu(), tol=GRAD_TOL)
        checked += 1
    assert checked >= 2 * (2 + 4 * L) + 8


def test_graph_capture_is_refused_for_a_homogeneous_model(tmp_path):
    from desco_amd.trainer import Trainer
    nm = on_gpu(homo_model(2, 64))
    with pytest.raises(NotImplementedError, match="--graph_capture does not support a homogeneous model"):
        Trainer(max_epochs=1, devices=[0], default_root_dir=str(tmp_path), graph_capture=True).fit(nm, datamodule=None)


# ---- 3. the driver and the inference pipeline -----------------------------------------------------------------------
def test_driver_trains_tests_and_predicts_and_the_pipeline_agrees(tmp_path):
    """``ablation_gnns.py`` in a fresh process: one epoch, two layers, on the MUTAG-shaped synthetic split; then
    InferencePipeline(nm, None, graphs) on the driver's best checkpoint against the driver's own prediction."""
    from desco_amd.data import load_data
    from desco_amd.pipeline import InferencePipeline
    out, ckpt, data = tmp_path / "out", tmp_path / "ckpt", tmp_path / "data"
    cmd = [sys.executable, os.path.join(ROOT, "ablation_gnns.py"), "--data_root", str(data),
           "--train_dataset", "MUTAG_train", "--valid_dataset", "MUTAG_val", "--test_dataset", "MUTAG_test",
           "--neigh_epoch_num", "1", "--neigh_layer_num", "2", "--neigh_batch_size", "64", "--neigh_model_path", str(ckpt),
           "--train_neigh", "--output_dir", str(out), "--seed", "0", "--gpu", "0"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    print(p.stdout[-1500:])
    cfg = (out / "config_MUTAG_test.txt").read_text()
    assert "use_hetero=False" in cfg and "use_tconv=False" in cfg and "conv_type='SAGE'" in cfg and "layer_num=2" in cfg
    best = re.search(r"best neighborhood model path:\s+(\S+)", p.stdout).group(1)
    assert os.path.exists(best) and (ckpt / "last.ckpt").exists()
    back = NeighborhoodCountingModel.load_from_checkpoint(best)
    assert back.emb_model.gnn_core.node_types is None and back.args.use_hetero is False
    assert "emb_model.gnn_core.convs.1.lin.weight" in back.state_dict()
    nums = lambda tag: [float(v) for v in re.search(tag + r": \[(.*?)\]", p.stdout).group(1).split(",")]   # noqa: E731
    norm_mse, mae = nums("graphlet_norm_mse_neighborhood"), nums("graphlet_mae_neighborhood")
    assert len(norm_mse) == len(mae) == 3 and np.isfinite(norm_mse).all() and np.isfinite(mae).all()
    val = float(re.search(r"final neighborhood_counting_val_loss: (\S+)", p.stdout).group(1))
    test = float(re.search(r"'test_loss': ([0-9.eE+-]+)", p.stdout).group(1))
    assert np.isfinite(val) and np.isfinite(test)
    # the homogeneous caches were written beside (not over) any hetero ones
    assert (data / "MUTAG_test" / "NeighborhoodDataset" / "processed" / "neighs_csr_depth_4_homo.npz").exists()
    driver_pred = pd.read_csv(out / "neighborhood_node_MUTAG_test_results.csv", index_col=0).to_numpy(dtype=np.float32)
    assert np.isfinite(driver_pred).all()
    # the pipeline picks the restricted builder from the model's args and runs without a gossip stage
    back = back.to(DEV)
    back.set_queries(standard_queries()[0], hetero=False)
    graphs = load_data("MUTAG_test", root_folder=str(data))
    pipe = InferencePipeline(back, None, graphs, depth=4, device=DEV)
    assert pipe.partition_backend == "device" and pipe.restricted and pipe.partition.restricted
    res = pipe.run(gossip=False)
    assert set(res) == {"neigh_count", "graph_neigh_count"}
    assert res["neigh_count"].shape == driver_pred.shape
    assert_counts_close("pipeline against the driver's prediction", res["neigh_count"], torch.from_numpy(driver_pred))
    with pytest.raises(ValueError, match="needs a gossip model"):
        pipe.run(gossip=True)
