"""CPU restatement of the HOMOGENEOUS neighborhood model (the reference's ablation_gnns.py configuration: use_hetero
False), in the reference's own form -- gnn_model.py:58-109 and :230-277 with ``self.use_hetero`` False:

    x = pre_mp(node_feature); per layer  x = relu(updates[l](cat(convs[l].lin(index_add_(x[src] at dst)), x)))  [* mask];
    emb = cat of all x;  emb[node_feature[:, 0] == 1] = anchor_mlp(those rows);  global_add_pool;  post_mp

with ONE pre_mp / convs[l].lin / updates[l] for every node and edge.  The head and both losses are the oracle's
(oracle.model.head_logits / train_loss_from_logits / eval_loss_from_logits).  Differentiable (torch autograd).

``tied_hetero_state_dict`` expands a homogeneous state dict into the hetero ``use_tconv=False`` one that computes the same
function; tests/test_homo_reference_host.py holds this restatement to the oracle's hetero path through it."""
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import model as OM
from oracle import partition as OP

UNION_EDGE_TYPES = (("count", "union", "canonical"), ("canonical", "union", "count"), ("count", "union", "count"))
QUERY_UNION = (("union_node", "union", "union_node"),)


# ---- the neighborhoods ----------------------------------------------------------------------------------------------
def restricted_neighborhoods(graphs, depth: int):
    """[(graph id, v, nodes ascending (v last), induced edges a < b)] of get_neigh_canonical (data.py:341-372) for every
    node whose neighborhood has an edge, in (graph, node) order."""
    out = []
    for gid, (n, edges) in enumerate(graphs):
        adj = OP.adjacency(n, edges)
        for v in range(n):
            seen, front = {v}, {v}
            for _ in range(depth):
                front = {w for u in front for w in adj[u] if w <= v} - seen
                seen |= front
            es = sorted((a, b) for a in seen for b in adj[a] if b in seen and a < b)
            if es:
                out.append((gid, v, sorted(seen), es))
    return out


def homo_batch(neighs) -> Dict:
    """The collated homogeneous batch of ``neighs`` [(nodes, edges)] with the anchor = the LAST node of each: rows in
    neighborhood order; node_feature [N, 1] (1 on the anchor), edge_index [2, E] (both directions), batch [N]."""
    feat, batch, src, dst, off = [], [], [], [], 0
    for g, (nodes, edges) in enumerate(neighs):
        loc = {v: off + i for i, v in enumerate(nodes)}
        feat += [0.0] * (len(nodes) - 1) + [1.0]
        batch += [g] * len(nodes)
        for a, b in edges:
            src += [loc[a], loc[b]]
            dst += [loc[b], loc[a]]
        off += len(nodes)
    return {"node_feature": torch.tensor(feat).view(-1, 1), "batch": torch.tensor(batch, dtype=torch.long),
            "edge_index": torch.tensor([src, dst], dtype=torch.long).view(2, -1), "num_graphs": len(neighs)}


def homo_query_batch(queries) -> Dict:
    """The query graphs with all-zero features (lightning_model.py:72-79): no row is an anchor"""
    b = homo_batch([(list(range(n)), sorted(tuple(sorted(e)) for e in es)) for n, es in queries])
    b["node_feature"] = torch.zeros_like(b["node_feature"])
    return b


def partition_rows(part) -> np.ndarray:
    """For a NeighborhoodPartition over the same neighborhoods: the row of ``homo_batch`` (neighborhood order, ascending
    ids, anchor last) that each row of the partition's layout (all count rows, then the canonical rows) holds -- valid
    for the builder's row order, NOT after degree_sorted()."""
    cp = part.count_ptr.astype(np.int64)
    B = part.num_neigh
    start = cp[:-1] + np.arange(B)                             # first homo row of neighborhood b
    count = np.concatenate([start[b] + np.arange(cp[b + 1] - cp[b]) for b in range(B)]) if B else np.zeros(0, np.int64)
    return np.concatenate([count, start + (cp[1:] - cp[:-1])]).astype(np.int64)


# ---- the model ------------------------------------------------------------------------------------------------------
def _lin(sd, key, x):
    return F.linear(x, sd[key + ".weight"], sd[key + ".bias"])


def base_gnn_homo(sd, prefix, batch: Dict, layer_num: int, masks=None):
    """BaseGNN.forward with use_hetero False.  ``masks`` = (layer_masks, post_mask): layer_masks[l] [N, H] are the
    dropout factors behind layer l's relu in the batch's row order, post_mask [B, H] those of post_mp.1."""
    feat, ei = batch["node_feature"], batch["edge_index"]
    core = prefix + ".gnn_core"
    x = _lin(sd, core + ".pre_mp.0", feat)                                             # :231
    emb = x
    for l in range(layer_num):
        agg = torch.zeros_like(x).index_add_(0, ei[1], x[ei[0]])                       # SAGEConv: add at edge_index[1]
        x_neigh = _lin(sd, f"{core}.convs.{l}.lin", agg)                               # :262
        x = F.relu(_lin(sd, f"{core}.updates.{l}", torch.cat((x_neigh, x), dim=1)))    # :264, :273
        if masks is not None and masks[0] is not None:
            x = x * masks[0][l]                                                        # :274
        emb = torch.cat((emb, x), dim=1)                                               # :275
    anchor = feat[:, 0] == 1                                                           # :77-83
    if bool(anchor.any()):
        idx = anchor.nonzero().view(-1)
        emb = emb.index_copy(0, idx, F.leaky_relu(_lin(sd, prefix + ".anchor_mlp.0", emb[idx]), 0.1))
    pooled = torch.zeros(batch["num_graphs"], emb.shape[1], dtype=emb.dtype).index_add_(0, batch["batch"], emb)   # :107
    return OM.post_mp(sd, prefix, pooled, None if masks is None else masks[1])         # :108


def homo_logits(sd, batch, qbatch, layer_num, masks_t=None, masks_q=None):
    """(target embeddings, [B, Q] logits) of graph_to_count / train_forward"""
    emb_q = base_gnn_homo(sd, "emb_model_query", qbatch, layer_num, masks_q)
    emb_t = base_gnn_homo(sd, "emb_model", batch, layer_num, masks_t)
    return emb_t, OM.head_logits(sd, emb_t, emb_q)


# ---- the untied twin ------------------------------------------------------------------------------------------------
def tied_hetero_state_dict(sd: Dict[str, torch.Tensor], layer_num: int) -> Dict[str, torch.Tensor]:
    """The hetero ``use_tconv=False`` state dict (to_hetero_old(False, False) key names) whose per-type / per-relation
    weights are copies of the homogeneous model's shared ones.

    One difference is forced by the two forms: a homogeneous SAGEConv adds its bias ONCE per destination row, to_hetero
    sums one SAGEConv per relation into a destination, each with a bias of its own -- so the count destinations (two
    relations: count -> count, canonical -> count) carry the bias on count -> count and ZERO on canonical -> count."""
    out = {}
    for k, v in sd.items():
        if ".gnn_core." not in k:
            out[k] = v
            continue
        prefix, rest = k.split(".gnn_core.")
        query = prefix == "emb_model_query"
        types = ("union_node",) if query else ("count", "canonical")
        ets = QUERY_UNION if query else UNION_EDGE_TYPES
        parts = rest.split(".")
        if parts[0] == "pre_mp":                                  # pre_mp.0.{weight,bias}
            for t in types:
                out[f"{prefix}.gnn_core.pre_mp.0.{t}.{parts[2]}"] = v
        elif parts[0] == "updates":                               # updates.l.{weight,bias}
            for t in types:
                out[f"{prefix}.gnn_core.updates.{parts[1]}.{t}.{parts[2]}"] = v
        elif parts[0] == "convs":                                 # convs.l.lin.{weight,bias}
            for (s, r, d) in ets:
                zero = parts[3] == "bias" and (s, d) == ("canonical", "count")
                out[f"{prefix}.gnn_core.convs.{parts[1]}.{s}__{r}__{d}.lin.{parts[3]}"] = v * 0 if zero else v
        else:
            raise KeyError(k)
    return out


def hetero_feats(batch_hetero: Dict) -> Dict[str, torch.Tensor]:
    """the 0/1 anchor feature per node type of an oracle hetero batch"""
    return {"count": torch.zeros(batch_hetero["num_nodes"]["count"], 1),
            "canonical": torch.ones(batch_hetero["num_nodes"]["canonical"], 1)}
