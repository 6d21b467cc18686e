"""Host-side checks of the plain GIN / GCN models (--neigh_conv_type GIN / GCN, ablation_gnns.py): the CPU restatement
(tests/plain_reference.py) against the homogeneous SAGE restatement (tests/homo_reference.py) on state dicts that make a
SAGE layer compute a GCN / GIN one, the state dict and checkpoint round trip of the model classes, the refusals, and the
zero padding -- of the restatement and of the packed operands (the ``+1`` fold of gnn_model.pack_plain)."""
import argparse

import pytest
import torch

import homo_reference as HR
import plain_reference as PR
from helpers import cpu_sd, golden_graphs, neigh_args, standard_queries
from test_homo_reference_host import FIVE_CYCLE

from desco_amd import gnn_model as GM
from desco_amd.lightning_model import NeighborhoodCountingModel


def plain_model(conv, layer_num=2, hidden=64, seed=0, dropout=0.0, gain=1.0, eps=None, **over):
    """A seeded plain model of the model class's own init (GIN: default nn.Linear; GCN: glorot weight, zero bias),
    the matrices multiplied by ``gain`` and 0.1 noise added to every bias, as helpers.make_models does; ``eps``: the
    value written into GIN's eps buffers."""
    torch.manual_seed(seed)
    args = argparse.Namespace(**{**vars(neigh_args(layer_num=layer_num, hidden_dim=hidden, dropout=dropout)),
                                 "use_hetero": False, "use_tconv": False, "use_canonical": True, "conv_type": conv, **over})
    nm = NeighborhoodCountingModel(1, hidden, args)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in nm.parameters():
            if p.dim() == 2:
                p.mul_(gain)
            else:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        if eps is not None:
            for name, b in nm.named_buffers():
                if name.endswith(".eps"):
                    b.fill_(eps)
    return nm


def _case(depth=3, n_graphs=6):
    graphs = [FIVE_CYCLE] + golden_graphs(max_n=30)[:n_graphs]
    _, queries = standard_queries()
    neighs = HR.restricted_neighborhoods(graphs, depth)
    assert len(neighs) > 40
    return HR.homo_batch([(nodes, es) for _, _, nodes, es in neighs]), HR.homo_query_batch(queries)


def _double(b):
    return dict(b, node_feature=b["node_feature"].double())


def _in_float64(f):
    torch.set_default_dtype(torch.float64)
    try:
        return f()
    finally:
        torch.set_default_dtype(torch.float32)


# ---- the restatement against the SAGE one ---------------------------------------------------------------------------
@pytest.mark.parametrize("layer_num", [2, 8])
def test_gcn_restatement_equals_the_sage_one_on_identity_updates(layer_num):
    """float64: SAGE with updates.l = [I | 0], zero bias, convs.l.lin = (W, b) is the GCN layer, to rounding"""
    hb, qb = _case()
    sd = {k: v.double() for k, v in cpu_sd(plain_model("GCN", layer_num)).items()}
    sage = PR.sage_state_dict_of(sd, layer_num, "GCN")

    def run():
        got = PR.plain_logits(sd, _double(hb), _double(qb), layer_num, "GCN")
        ref = HR.homo_logits(sage, _double(hb), _double(qb), layer_num)
        return got, ref
    (emb, logits), (ref_emb, ref_logits) = _in_float64(run)
    assert float(ref_emb.std(0).mean()) > 1e-3, "embeddings do not depend on the neighborhood"
    assert float((emb - ref_emb).abs().max()) <= 1e-10 * max(float(ref_emb.abs().max()), 1.0)
    assert float((logits - ref_logits).abs().max()) <= 1e-10 * max(float(ref_logits.abs().max()), 1.0)


@pytest.mark.parametrize("eps", [0.0, 0.25])
@pytest.mark.parametrize("layer_num", [2, 8])
def test_gin_restatement_equals_the_sage_one_when_the_second_linear_is_the_identity(layer_num, eps):
    """float64: GIN with updates.l.2 = (I, 0) is SAGE with convs.l.lin = (W1, b1 + W1 1), updates.l = [I | eps W1] -- the
    constant 1 of ``x_neigh + (1 + eps x)`` lands in the bias, the row's own features enter through eps alone"""
    hb, qb = _case()
    sd = {k: v.double() for k, v in cpu_sd(plain_model("GIN", layer_num, eps=eps)).items()}
    for k in list(sd):
        if ".updates." in k and ".2." in k:
            sd[k] = torch.eye(64, dtype=torch.float64) if k.endswith("weight") else torch.zeros(64, dtype=torch.float64)
    sage = PR.sage_state_dict_of(sd, layer_num, "GIN")

    def run():
        got = PR.plain_logits(sd, _double(hb), _double(qb), layer_num, "GIN")
        ref = HR.homo_logits(sage, _double(hb), _double(qb), layer_num)
        return got, ref
    (emb, logits), (ref_emb, ref_logits) = _in_float64(run)
    assert float(ref_emb.std(0).mean()) > 1e-3
    assert float((emb - ref_emb).abs().max()) <= 1e-10 * max(float(ref_emb.abs().max()), 1.0)
    assert float((logits - ref_logits).abs().max()) <= 1e-10 * max(float(ref_logits.abs().max()), 1.0)
    if eps:         # the row's own features matter only through eps
        sd0 = {k: (v * 0 if k.endswith(".eps") else v) for k, v in sd.items()}
        other = _in_float64(lambda: PR.plain_logits(sd0, _double(hb), _double(qb), layer_num, "GIN")[0])
        assert float((other - emb).abs().max()) > 1e-6


# ---- model surface --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [64, 100])
@pytest.mark.parametrize("conv", PR.CONVS)
def test_state_dict_keys_shapes_and_checkpoint_round_trip(tmp_path, conv, hidden):
    L = 3
    nm = plain_model(conv, L, hidden, eps=0.25 if conv == "GIN" else None)
    sd = nm.state_dict()
    h = hidden
    for m in ("emb_model", "emb_model_query"):
        core = m + ".gnn_core"
        assert tuple(sd[core + ".pre_mp.0.weight"].shape) == (h, 1)
        ck = [k for k in sd if k.startswith(core + ".") and ".pre_mp." not in k]
        want = {}
        for l in range(L):
            if conv == "GIN":
                want.update({f"{core}.updates.{l}.0.weight": (h, h), f"{core}.updates.{l}.0.bias": (h,),
                             f"{core}.updates.{l}.2.weight": (h, h), f"{core}.updates.{l}.2.bias": (h,),
                             f"{core}.eps.{l}.eps": (1,)})
            else:
                want.update({f"{core}.convs.{l}.lin.weight": (h, h), f"{core}.convs.{l}.bias": (h,)})
        assert {k: tuple(sd[k].shape) for k in ck} == want
        if conv == "GIN":
            assert not any(".convs." in k for k in ck)                       # GINConv never stores its nn
            params = dict(nm.named_parameters())
            assert all(f"{core}.eps.{l}.eps" not in params for l in range(L))  # a buffer, not a parameter
        else:
            assert not any(".updates." in k or "lin.bias" in k for k in ck)
            c = getattr(nm, m).gnn_core.convs[0]
            bound = (6.0 / (2 * h)) ** 0.5                                   # glorot
            fresh = GM.GCNConv(h, h)
            assert float(fresh.lin.weight.detach().abs().max()) <= bound and not fresh.bias.any() and c.lin.bias is None
        assert tuple(sd[m + ".anchor_mlp.0.weight"].shape) == ((L + 1) * h, (L + 1) * h)
    core = nm.emb_model.gnn_core
    assert core.is_plain() and core.is_homogeneous() and nm.emb_model.is_wide() and core.node_types is None
    assert core.row_types() == ["count", "canonical"] and nm.emb_model_query.gnn_core.row_types() == ["union_node"]
    path = str(tmp_path / "plain.ckpt")
    nm.save_checkpoint(path)
    back = NeighborhoodCountingModel.load_from_checkpoint(path)
    assert back.args.conv_type == conv and back.args.use_hetero is False and back.emb_model.gnn_core.is_plain()
    a, b = nm.state_dict(), back.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    if conv == "GIN":
        assert all(float(b[f"emb_model.gnn_core.eps.{l}.eps"]) == 0.25 for l in range(L))


def test_refusals_name_the_flag():
    flag = "--neigh_conv_type"
    for conv in ("GIN", "GCN"):
        with pytest.raises(NotImplementedError, match=flag + ".*ablation_gnns.py"):        # hetero GIN / GCN (main.py)
            NeighborhoodCountingModel(1, 64, neigh_args(layer_num=2, conv_type=conv))
        nm = plain_model(conv)
        with pytest.raises(NotImplementedError, match=flag):                               # to_hetero of a plain core
            nm.to_hetero_old(False, False)
        with pytest.raises(NotImplementedError, match=flag):
            nm.emb_model.gnn_core.to_hetero(GM.QUERY_NODE_TYPES, GM.QUERY_EDGE_TYPES_UNION)
    for conv in ("GAT", "PNACONV"):
        for hetero in (True, False):
            with pytest.raises(NotImplementedError, match=flag):
                NeighborhoodCountingModel(1, 64, neigh_args(layer_num=2, conv_type=conv, use_hetero=hetero))
    import ablation_gnns
    ns = argparse.Namespace
    with pytest.raises(NotImplementedError, match=flag + " GAT"):
        ablation_gnns.main(ns(conv_type="GAT"), ns(), ns(gpu=0), atlas_query_ids=[6])
    with pytest.raises(NotImplementedError, match=flag + " GIN"):
        ablation_gnns.main(ns(conv_type="GIN", use_node_feature=True), ns(), ns(gpu=0), atlas_query_ids=[6])
    with pytest.raises(NotImplementedError, match=flag + " GCN"):
        ablation_gnns.main(ns(conv_type="GCN"), ns(), ns(gpu=[0, 1]), atlas_query_ids=[6])


# ---- zero padding ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [32, 100])
@pytest.mark.parametrize("conv,eps", [("GIN", None), ("GIN", 0.25), ("GCN", None)])
def test_per_block_zero_padding_is_exact_on_the_restatement(conv, eps, h):
    """The restatement on the state dict padded block by block to wp equals the one on the true state dict, and the
    padded channels of every layer and of the embeddings are exactly 0 -- although GIN's constant 1 is added to the padded
    channels of z too: the padded input columns of updates.l.0 are zero."""
    L = 3
    hb, qb = _case(depth=4)
    nm = plain_model(conv, L, h, eps=eps)
    wp = GM.padded_width(h)
    sd = cpu_sd(nm)
    sdp = PR.padded_state_dict(sd, h, wp, L)
    emb, logits = PR.plain_logits(sd, hb, qb, L, conv)
    embp, logitsp = PR.plain_logits(sdp, hb, qb, L, conv)
    d = float((logitsp - logits).abs().max())
    print(f"[gate] padded-vs-true {conv} restatement logits at h={h}: max |d| = {d:.2e} (gate 1e-5)")
    assert d <= 1e-5 and float((embp[:, :h] - emb).abs().max()) <= 1e-5 and float(embp[:, h:].abs().max()) == 0.0
    for x, xp in zip(PR.plain_layers(sd, "emb_model", hb, L, conv), PR.plain_layers(sdp, "emb_model", hb, L, conv)):
        assert float(xp[:, h:].abs().max()) == 0.0 and float((xp[:, :h] - x).abs().max()) <= 1e-5 * (1 + float(x.abs().max()))


@pytest.mark.parametrize("h", [32, 64, 100])
@pytest.mark.parametrize("conv,eps", [("GIN", None), ("GIN", 0.25), ("GCN", None)])
def test_packed_operands_compute_the_restatement_with_the_one_folded_into_the_bias(conv, eps, h):
    """gnn_model.pack_plain(planes=False) evaluated with plain torch on the CPU -- z = agg + eps x, relu(z wt1 + b1)
    [relu(. wt2 + b2)] -- equals the restatement's layers: GIN's ``+1`` sits in b1 = b1 + W1 1 over the TRUE width, so
    the padded channels are exactly 0 (they would be relu(0 + 0) anyway; the sum over the padded columns adds nothing)"""
    L = 2
    hb, _ = _case(depth=4)
    nm = plain_model(conv, L, h, eps=eps)
    wp = GM.padded_width(h)
    with torch.no_grad():
        pk = GM.pack_plain(nm.emb_model, planes=False)
    assert pk["wp"] == wp and pk["h"] == h and len(pk["layers"]) == L
    assert pk["anchor"][0].shape == ((L + 1) * wp, (L + 1) * wp) and pk["post"][0][0].shape == ((L + 1) * wp, wp)
    ref = PR.plain_layers(cpu_sd(nm), "emb_model", hb, L, conv)
    ei = hb["edge_index"]
    x = hb["node_feature"] @ pk["pre"]["count"][0] + pk["pre"]["count"][1]
    assert pk["pre"]["canonical"][0] is pk["pre"]["count"][0]
    for l, e in enumerate(pk["layers"]):
        assert e["wt1"].shape == (wp, wp) and e["b1"].shape == (wp,)
        z = torch.zeros_like(x).index_add_(0, ei[1], x[ei[0]])
        if conv == "GIN":
            assert float(e["eps"]) == (eps or 0.0)
            z = z + e["eps"] * x
            x = torch.relu(torch.relu(z @ e["wt1"] + e["b1"]) @ e["wt2"] + e["b2"])
        else:
            assert "wt2" not in e and "eps" not in e
            x = torch.relu(z @ e["wt1"] + e["b1"])
        assert float(x[:, h:].abs().max()) == 0.0 if wp > h else True
        assert float((x[:, :h] - ref[l + 1]).abs().max()) <= 1e-5 * (1 + float(ref[l + 1].abs().max()))
    # gradients reach the true-width parameters through the padded operands, and eps gets none
    nm.zero_grad()
    pk = GM.pack_plain(nm.emb_model, planes=False)
    sum(float(i + 1) * (e["wt1"].sum() + e["b1"].sum()) for i, e in enumerate(pk["layers"])).backward()
    core = nm.emb_model.gnn_core
    first = core.updates[0][0] if conv == "GIN" else core.convs[0].lin
    assert first.weight.grad is not None and tuple(first.weight.grad.shape) == (h, h)
    if conv == "GIN":
        assert torch.allclose(first.weight.grad, torch.full((h, h), 2.0))      # once as wt1, once inside b1 = b1 + W1 1
        assert not core.eps[0].eps.requires_grad
