"""CPU restatement of the plain GIN and GCN neighborhood models (the reference's BaseGNN with use_hetero False and
--neigh_conv_type GIN / GCN: gnn_model.py:58-109, :230-277), in the reference's own form:

    x = pre_mp(node_feature); per layer, with agg = index_add_(x[src] at dst):
        GIN   x = relu(updates[l](agg + (1 + eps_l * x)))      updates[l] = Linear, ReLU, Linear; eps_l a buffer [1]
        GCN   x = relu(agg @ convs[l].lin.weight^T + convs[l].bias)                 (GCNConv(normalize=False))
    [* mask];  emb = cat of all x;  emb[node_feature[:, 0] == 1] = anchor_mlp(those rows);  global_add_pool;  post_mp

The GIN line is read as the reference writes it: the parentheses put the row's own features under eps, so that with
eps = 0 they drop out and a constant 1 is added to every channel.  Everything outside the layer loop, the batches, the
head and both losses are those of tests/homo_reference.py / oracle.model.  Differentiable (torch autograd); takes masks
like homo_reference.base_gnn_homo.  tests/test_plain_reference_host.py holds it to the homogeneous SAGE restatement
through state dicts that make the SAGE layer compute a GCN / GIN one."""
from typing import Dict

import torch
import torch.nn.functional as F

import homo_reference as HR
from oracle import model as OM

CONVS = ("GIN", "GCN")


def plain_layers(sd, prefix, batch: Dict, layer_num: int, conv: str, masks=None):
    """[x_0, ..., x_L] of BaseGNNCore.forward: the layer loop alone"""
    feat, ei = batch["node_feature"], batch["edge_index"]
    core = prefix + ".gnn_core"
    x = HR._lin(sd, core + ".pre_mp.0", feat)                                          # :231
    xs = [x]
    for l in range(layer_num):
        agg = torch.zeros_like(x).index_add_(0, ei[1], x[ei[0]])                       # propagate, aggr="add"
        if conv == "GIN":
            z = agg + (1 + sd[f"{core}.eps.{l}.eps"] * x)                              # :266, as written
            x = HR._lin(sd, f"{core}.updates.{l}.2", F.relu(HR._lin(sd, f"{core}.updates.{l}.0", z)))
        else:
            assert conv == "GCN"
            x = F.linear(agg, sd[f"{core}.convs.{l}.lin.weight"]) + sd[f"{core}.convs.{l}.bias"]      # :268-270
        x = F.relu(x)                                                                  # :273
        if masks is not None and masks[0] is not None:
            x = x * masks[0][l]                                                        # :274
        xs.append(x)
    return xs


def base_gnn_plain(sd, prefix, batch: Dict, layer_num: int, conv: str, masks=None):
    """BaseGNN.forward with use_hetero False and conv_type ``conv``.  ``masks`` = (layer_masks, post_mask) as in
    homo_reference.base_gnn_homo."""
    feat = batch["node_feature"]
    emb = torch.cat(plain_layers(sd, prefix, batch, layer_num, conv, masks), dim=1)    # :275
    anchor = feat[:, 0] == 1                                                           # :77-83
    if bool(anchor.any()):
        idx = anchor.nonzero().view(-1)
        emb = emb.index_copy(0, idx, F.leaky_relu(HR._lin(sd, prefix + ".anchor_mlp.0", emb[idx]), 0.1))
    pooled = torch.zeros(batch["num_graphs"], emb.shape[1], dtype=emb.dtype).index_add_(0, batch["batch"], emb)   # :107
    return OM.post_mp(sd, prefix, pooled, None if masks is None else masks[1])         # :108


def plain_logits(sd, batch, qbatch, layer_num, conv, masks_t=None, masks_q=None):
    """(target embeddings, [B, Q] logits) of graph_to_count / train_forward"""
    emb_q = base_gnn_plain(sd, "emb_model_query", qbatch, layer_num, conv, masks_q)
    emb_t = base_gnn_plain(sd, "emb_model", batch, layer_num, conv, masks_t)
    return emb_t, OM.head_logits(sd, emb_t, emb_q)


# ---- SAGE state dicts that compute a plain layer (for the host checks) --------------------------------------------
def sage_state_dict_of(sd, layer_num: int, conv: str):
    """The homogeneous SAGE state dict whose layer  relu(updates[l](cat(convs[l].lin(agg), x)))  equals the plain one:
      GCN   convs.l.lin = (W, b),                updates.l = [I | 0], bias 0
      GIN   convs.l.lin = (W1, b1 + W1 1),       updates.l = [I | eps W1], bias 0      -- valid when updates.l.2 = (I, 0)"""
    out = {k: v for k, v in sd.items() if ".gnn_core.convs." not in k and ".gnn_core.updates." not in k
           and ".gnn_core.eps." not in k}
    for m in ("emb_model", "emb_model_query"):
        core = m + ".gnn_core"
        for l in range(layer_num):
            if conv == "GCN":
                Wm, b = sd[f"{core}.convs.{l}.lin.weight"], sd[f"{core}.convs.{l}.bias"]
                right = torch.zeros_like(Wm)
            else:
                Wm, b1 = sd[f"{core}.updates.{l}.0.weight"], sd[f"{core}.updates.{l}.0.bias"]
                h = Wm.shape[0]
                assert torch.equal(sd[f"{core}.updates.{l}.2.weight"], torch.eye(h, dtype=Wm.dtype))
                assert not sd[f"{core}.updates.{l}.2.bias"].any()
                b = b1 + Wm.sum(1)
                right = sd[f"{core}.eps.{l}.eps"] * Wm
            h = Wm.shape[0]
            out[f"{core}.convs.{l}.lin.weight"], out[f"{core}.convs.{l}.lin.bias"] = Wm, b
            out[f"{core}.updates.{l}.weight"] = torch.cat([torch.eye(h, dtype=Wm.dtype), right], 1)
            out[f"{core}.updates.{l}.bias"] = torch.zeros(h, dtype=Wm.dtype)
    return out


# ---- zero padding ---------------------------------------------------------------------------------------------------
def padded_state_dict(sd, h: int, wp: int, layer_num: int):
    """The state dict of the same plain model at width wp, every h-wide block zero-padded on its own"""
    L = layer_num
    pad = F.pad

    def to(v, *shape):
        pads = []
        for d in reversed(range(v.dim())):
            pads += [0, shape[d] - v.shape[d]]
        return pad(v, pads)
    out = {}
    for k, v in sd.items():
        v = v.clone()
        if k == "count_model.0.weight":
            v = to(pad(v.view(v.shape[0], 2, h), (0, wp - h)).reshape(v.shape[0], 2 * wp), 4 * wp, 2 * wp)
        elif k in ("count_model.0.bias", "count_model.2.weight"):
            v = to(v, *([4 * wp] if v.dim() == 1 else [1, 4 * wp]))
        elif k == "count_model.2.bias" or ".eps." in k:
            pass
        elif "anchor_mlp.0" in k:
            v = pad(v.view(L + 1, h, L + 1, h), (0, wp - h, 0, 0, 0, wp - h)).reshape((L + 1) * wp, (L + 1) * wp) \
                if v.dim() == 2 else pad(v.view(L + 1, h), (0, wp - h)).reshape(-1)
        elif "post_mp.0" in k:
            v = to(pad(v.view(h, L + 1, h), (0, wp - h)).reshape(h, -1), wp, (L + 1) * wp) if v.dim() == 2 else to(v, wp)
        elif "post_mp." in k:
            v = to(v, *[wp if d == h else d for d in v.shape])
        elif "pre_mp" in k:
            v = to(v, wp, v.shape[1]) if v.dim() == 2 else to(v, wp)
        elif ".updates." in k or ".convs." in k:
            v = to(v, wp, wp) if v.dim() == 2 else to(v, wp)
        else:
            raise AssertionError(f"unexpected key {k}")
        out[k] = v
    return out
