"""GNN building blocks with the reference's names, parameters and state-dict keys
(subgraph_counting/gnn_model.py:18-419), executing on MI355X through libdesco_hip.so.

The modules only HOLD parameters in the reference's layout (so the authors' checkpoints load);
``forward`` does not run them as torch layers.  Instead the weights are folded ("packed") into the
operands of the HIP kernels:

  SHMP layer (SAGEConv x edge types + to_hetero sum + updates Linear, gnn_model.py:262-264, 395):
      x'_d = relu( sum_s agg_s (U_n W_s)^T + x_d U_x^T + (U_n sum_s b_s + c) )
      -> one gather kernel + one MFMA GEMM with K = (S+1)*64 per destination type.
  Gossip (GossipConv, gnn_model.py:280-350): see ``gossip_forward`` and DESIGN.md section 4.2.

There is no CPU / eager fallback: inputs must live on the GPU.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Dict, List, Optional, Sequence, Tuple

import os

import torch
import torch.nn as nn

from . import ops
from .batch import GossipBatch, GraphBatch, NeighborhoodBatch, QueryBatch

H = 64
# the fused gossip pass in the three-product fp16 form (csrc/gossip_f16.hip); False: the six-product bf16 kernel
# (csrc/gossip_fused.hip), kept as its cross-check
GOSSIP_F16X3 = os.environ.get("DESCO_GOSSIP_F16X3", "1") != "0"
# inference GEMMs (anchor, post MLP, head, canonical table) on the bf16 matrix pipe with fp32-level
# accuracy (bf16x6 split, csrc/gemm_split.hip); False: v_mfma_f32_32x32x2_f32 (gemm_f32.hip)
GEMM_BF16X6 = True
# the large inference GEMM (anchor MLP) in the THREE-product fp16 hi/lo form (csrc/gemm_f16x3.hip): half the MFMAs and
# two operand planes instead of three, power-of-two scales per weight matrix and per activation row; measured error
# below the f32 MFMA's (tests/test_kernels_gpu.py::test_gemm_f16x3_is_fp32_accurate).  Needs GEMM_BF16X6.
GEMM_F16X3 = os.environ.get("DESCO_GEMM_F16X3", "1") != "0"
# True: the fused SHMP layer's MFMA blocks also run as the bf16x6 split (csrc/shmp_layer.hip, K <= 192)
SHMP_BF16X6 = True
# ... in the three-product fp16 form with per-row power-of-two scales (csrc/shmp_layer16.hip, F16 instantiations); needs
# SHMP_BF16X6 and 16-row wave tiles
SHMP_F16X3 = os.environ.get("DESCO_SHMP_F16X3", "1") != "0"
# the closed-form first layer's count launch leaves pooled partial sums (desco_degree_affine_pool_f32) like the fused
# layer launches do, instead of a segment-sum pass over the rows it has just written
POOL_FIRST_LAYER = os.environ.get("DESCO_POOL_FIRST_LAYER", "1") != "0"
# the canonical rows of every layer are stored ONCE, in their column block of the anchor operand [B, 64 (L + 1)]: the
# canonical launches read their own rows from there (desco_shmp_layer_f16x3_f32: xself) and the table products too,
# instead of from a second copy behind the count rows of X_l (False: both copies, rounds 2-5)
CANON_ROWS_ONCE = os.environ.get("DESCO_CANON_ROWS_ONCE", "1") != "0"
# degree-balanced row order inside the fused gossip kernel's 128-node tiles (desco_gossip_tile_order); results are
# bit-identical with and without it
GOSSIP_TILE_ORDER = os.environ.get("DESCO_GOSSIP_TILE_ORDER", "1") != "0"
# the f16x3 gossip pass through the planned kernel (desco_gossip_planned_f16x3_f32: per-batch plan, packed operands,
# buffer loads) wherever its 32-bit bound holds (ops.gossip_plan_fits); results are bit-identical either way.
# DESCO_GOSSIP_PLAN=0: the launches of desco_gossip_fused_f16x3_f32 everywhere.
GOSSIP_PLAN = os.environ.get("DESCO_GOSSIP_PLAN", "1") != "0"
_RELEASED = object()        # placeholder of a layer's rows that shmp_forward has released

TARGET_NODE_TYPES = ["count", "canonical"]
# metadata of to_hetero_old(tconv_target=True), lightning_model.py:376-383
TARGET_EDGE_TYPES_TCONV = [
    ("count", "union_triangle", "count"),
    ("count", "union_tride", "count"),
    ("count", "union_triangle", "canonical"),
    ("count", "union_tride", "canonical"),
    ("canonical", "union_triangle", "count"),
    ("canonical", "union_tride", "count"),
]
# lightning_model.py:392-397
TARGET_EDGE_TYPES_UNION = [
    ("count", "union", "canonical"),
    ("canonical", "union", "count"),
    ("count", "union", "count"),
]
QUERY_NODE_TYPES = ["union_node"]
QUERY_EDGE_TYPES_TCONV = [
    ("union_node", "union_triangle", "union_node"),
    ("union_node", "union_tride", "union_node"),
]
QUERY_EDGE_TYPES_UNION = [("union_node", "union", "union_node")]
# a homogeneous core (use_hetero=False) serves every row type of the batches with its one set of weights
HOMO_ROW_TYPES = ["count", "canonical", "union_node"]
HOMO_KEY = "lin"


# widths of the neighborhood / query models (--neigh_hidden_dim): H == 64 runs the fused kernels; any other width up to
# MAX_HIDDEN runs the wide path (shmp_forward_wide) on operands zero-padded to padded_width(H)
MAX_HIDDEN = 256


def padded_width(h: int) -> int:
    """the width the kernels see: 64 ceil(h / 64)"""
    return 64 * ((int(h) + 63) // 64)


def _require_hidden(hidden_dim, conv_type="SAGE", emb_channels=None):
    if conv_type == "GOSSIP":
        if hidden_dim != H:
            raise NotImplementedError(
                f"--gossip_hidden_dim must be {H} (the gossip kernels are specialised for it); got {hidden_dim}")
        if emb_channels is not None and not 1 <= int(emb_channels) <= MAX_HIDDEN:
            raise NotImplementedError(
                f"--neigh_hidden_dim (the gossip model's emb_channels) must be in 1..{MAX_HIDDEN}; got {emb_channels}")
        return
    if not 1 <= int(hidden_dim) <= MAX_HIDDEN:
        raise NotImplementedError(f"--neigh_hidden_dim must be in 1..{MAX_HIDDEN}; got {hidden_dim}")


class SAGEConv(nn.Module):
    """Sum-aggregate then Linear (gnn_model.py:362-419).  Holds ``lin``."""

    def __init__(self, in_channels, out_channels, aggr="add", **kwargs):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = nn.Linear(in_channels, out_channels)

    def reset_parameters(self):
        self.lin.reset_parameters()

    def forward(self, x, edge_index, edge_weight=None, size=None, res_n_id=None):
        """Stand-alone call with PyG semantics (gnn_model.py:372-400) on device tensors."""
        if isinstance(x, torch.Tensor):
            x = (x, x)
        x_src, x_dst = x
        n_dst = x_dst.shape[0] if size is None else size[1]
        if edge_index is None:
            edge_index = torch.zeros((2, 0), dtype=torch.long, device=x_src.device)
        if edge_index.numel() != 0:
            edge_index = edge_index[:, edge_index[0] != edge_index[1]]     # :389-390
        dst, order = torch.sort(edge_index[1])
        col = edge_index[0][order].to(torch.int32)
        rowptr = torch.zeros(n_dst + 1, dtype=torch.int64, device=x_src.device)
        rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n_dst), 0)
        agg = ops.csr_gather_sum(x_src.float().contiguous(), rowptr.to(torch.int32), col, n_dst, 1)
        return ops.gemm(agg, self.lin.weight.t().contiguous(), self.lin.bias)

    def __repr__(self):
        return "{}({}, {})".format(self.__class__.__name__, self.in_channels, self.out_channels)


# plain layer types of a homogeneous core (--neigh_conv_type GIN / GCN, ablation_gnns.py)
PLAIN_CONV_TYPES = ("GIN", "GCN")


def _plain_aggregate(x: torch.Tensor, edge_index, n_dst: int) -> torch.Tensor:
    """agg[i] = sum of x[src] over the edges into i (PyG ``propagate`` with aggr="add"; no self loops are added or
    removed) for x of a width % 4 == 0 up to MAX_HIDDEN, on desco_csr_gather_sum_wide_f32"""
    if edge_index is None:
        edge_index = torch.zeros((2, 0), dtype=torch.long, device=x.device)
    dst, order = torch.sort(edge_index[1], stable=True)
    col = edge_index[0][order].to(torch.int32)
    rowptr = torch.zeros(n_dst + 1, dtype=torch.int64, device=x.device)
    rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n_dst), 0)
    return ops.csr_gather_sum_wide(x.float().contiguous(), rowptr.to(torch.int32), col, n_dst, 1)


class GINConv(nn.Module):
    """The reference's GINConv (gnn_model.py:422-446): sum aggregation and nothing else -- the ``nn`` handed to it is
    never stored, the (1 + eps) x term is commented out there.  Holds NO parameters (no ``convs.l.*`` keys)."""

    def __init__(self, in_channels, out_channels, aggr="add", **kwargs):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels

    def forward(self, x, edge_index, size=None):
        return _plain_aggregate(x, edge_index, x.shape[0] if size is None else size[1])

    def __repr__(self):
        return "{}({}, {})".format(self.__class__.__name__, self.in_channels, self.out_channels)


class GINEps(nn.Module):
    """The reference's TrivalParam (gnn_model.py:449-460): the BUFFER ``eps`` of shape [1] (key ``eps.l.eps``)"""

    def __init__(self, n=0.0):
        super().__init__()
        self.n = n
        self.register_buffer("eps", torch.tensor([float(n)]))

    def forward(self) -> torch.Tensor:
        return self.eps

    def reset_parameters(self):
        self.eps.data.fill_(self.n)


class GCNConv(nn.Module):
    """pyg_nn.GCNConv(i, h, normalize=False) of PyG 2.2.0, restated (PyG-only semantics, unpinned: DESIGN.md 2):
    ``lin`` = Linear without bias (glorot), ``bias`` [h] (zeros); out = (sum of x_j over the row's neighbours) lin^T +
    bias -- with normalize=False neither self loops nor a normalisation are added."""

    def __init__(self, in_channels, out_channels, aggr="add", **kwargs):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.lin.weight)          # torch_geometric.nn.inits.glorot
        nn.init.zeros_(self.bias)

    def forward(self, x, edge_index, size=None):
        wp = padded_width(self.in_channels)
        agg = _plain_aggregate(torch.nn.functional.pad(x.float(), (0, wp - x.shape[1])), edge_index,
                               x.shape[0] if size is None else size[1])
        return ops.gemm(agg, _pad_to(self.lin.weight.t(), wp, padded_width(self.out_channels)).contiguous(),
                        _pad_to(self.bias, padded_width(self.out_channels)).contiguous())[:, :self.out_channels]

    def __repr__(self):
        return "{}({}, {})".format(self.__class__.__name__, self.in_channels, self.out_channels)


class GossipConv(nn.Module):
    """Direction-gated message passing conditioned on the query embedding (gnn_model.py:280-359).
    Holds ``lin_com``, ``lin_update``, ``lin_gate``; executed by ``gossip_forward``."""

    def __init__(self, in_channels, out_channels, emb_channels, aggr="add", **kwargs):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin_com = nn.Linear(in_channels, out_channels)
        self.lin_update = nn.Linear(out_channels + in_channels, out_channels)
        self.lin_gate = nn.Sequential(
            nn.Linear(emb_channels, out_channels), nn.Sigmoid(),
            nn.Linear(out_channels, 1), nn.Sigmoid(), nn.LeakyReLU())

    def _gate_value(self, query_emb: torch.Tensor):
        """lin_gate(query_emb) (gnn_model.py:294-301, 357-359) -> [Q, 1].  Written out: the 64 -> 1 Linear as a product
        and a row sum instead of a matrix-vector product (rocBLAS gemv reduces with float atomics: see ``_mv``)."""
        l0, l2 = self.lin_gate[0], self.lin_gate[2]
        h = torch.sigmoid(torch.nn.functional.linear(query_emb, l0.weight, l0.bias))
        g = torch.sigmoid((h * l2.weight[0]).sum(-1, keepdim=True) + l2.bias)
        return torch.nn.functional.leaky_relu(g, self.lin_gate[4].negative_slope)

    def forward(self, x, edge_index, edge_weight=None, size=None, res_n_id=None, query_emb=None):
        """Stand-alone layer call with the reference's semantics (gnn_model.py:303-350) on device
        tensors, for ONE query: ``out = lin_update([sum_j w_ji * lin_com(x_j) | x])`` with
        ``w_ji = gate`` where ``edge_weight`` is True and ``1 - gate`` elsewhere.  (The model path
        does not call this: ``BaseGNN.forward`` batches all queries and both layers into the fused
        kernels.)  ``edge_weight`` must be the direction flag ``src < dst`` the reference computes
        (gnn_model.py:246-248); it is derived when omitted."""
        if edge_index.numel():
            edge_index = edge_index[:, edge_index[0] != edge_index[1]]          # remove_self_loops
        src, dst = edge_index[0], edge_index[1]
        if edge_weight is None:
            both = torch.cat([edge_index, edge_index.flip(0)], 1)               # to_undirected
            both = torch.unique(both, dim=1)
            src, dst = both[0], both[1]
        elif not torch.equal(edge_weight.bool(), src < dst):
            raise NotImplementedError("GossipConv.forward: edge_weight must be the flag src < dst")
        n = x.shape[0]
        gate = 0.5 if query_emb is None else float(self.lin_gate(query_emb.reshape(1, -1)).detach().reshape(()))
        order = torch.argsort(dst, stable=True)
        col = src[order].to(torch.int32)
        rowptr = torch.zeros(n + 1, dtype=torch.int64, device=x.device)
        rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n), 0)
        msg = ops.gemm(x.float().contiguous(), self.lin_com.weight.t().contiguous(), self.lin_com.bias)
        g = torch.tensor([gate], device=x.device, dtype=torch.float32)
        agg = ops.gossip_gather(msg, rowptr.to(torch.int32), col, n, 1, g)      # [n, 64]
        return ops.gemm(agg, self.lin_update.weight.t().contiguous(), self.lin_update.bias,
                        a2=x.float().contiguous())

    def __repr__(self):
        return "{}({}, {})".format(self.__class__.__name__, self.in_channels, self.out_channels)


class BaseGNNCore(nn.Module):
    """pre_mp + L x (conv, update) (gnn_model.py:115-277).  ``to_hetero`` re-creates PyG's
    per-node-type / per-edge-type module copies with its state-dict naming
    ("__".join(edge_type))."""

    def __init__(self, input_dim, hidden_dim, output_dim, args, **kwargs):
        super().__init__()
        _require_hidden(hidden_dim, args.conv_type, kwargs.get("emb_channels"))
        self.hidden_dim = hidden_dim
        self.dropout = args.dropout
        self.layer_num = args.layer_num
        self.conv_type = args.conv_type
        self.use_hetero = args.use_hetero
        self.kwargs = kwargs
        self.input_dim = input_dim
        pre_dim_out = hidden_dim
        self.pre_mp = nn.Sequential(nn.Linear(input_dim, pre_dim_out))          # :131
        self.input_pattern_emb = "input_pattern_emb" in kwargs                  # :144-153
        if self.input_pattern_emb:
            pre_dim_out += kwargs["emb_channels"]
        self.convs = nn.ModuleList()
        self.updates = nn.ModuleList()
        if args.conv_type == "GIN":
            self.eps = nn.ModuleList()                                              # :141-143
        for l in range(args.layer_num):
            hidden_input_dim = hidden_dim
            if l == 0 and self.input_pattern_emb:
                hidden_input_dim = hidden_dim + kwargs["emb_channels"]
            if args.conv_type == "GOSSIP":
                self.convs.append(GossipConv(hidden_input_dim, hidden_dim,
                                             emb_channels=kwargs["emb_channels"]))        # :178-183
            elif args.conv_type == "SAGE":
                self.convs.append(SAGEConv(hidden_input_dim, hidden_dim, aggr="add"))     # :187
                self.updates.append(nn.Linear(2 * hidden_dim, hidden_dim))                # :190
            elif args.conv_type in PLAIN_CONV_TYPES:
                if args.use_hetero:
                    raise NotImplementedError(
                        f"--neigh_conv_type {args.conv_type} runs as a homogeneous model only (use_hetero=False: "
                        "ablation_gnns.py --neigh_conv_type " + args.conv_type + "); the heterogeneous (to_hetero) form "
                        "of a GIN / GCN core is not on the hot path")
                if self.input_pattern_emb:
                    raise NotImplementedError(f"--neigh_conv_type {args.conv_type}: no query embedding as input feature")
                if args.conv_type == "GIN":
                    self.convs.append(GINConv(hidden_input_dim, hidden_dim, aggr="add"))           # :186-187 (no parameters)
                    self.updates.append(nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.ReLU(),
                                                      nn.Linear(hidden_dim, hidden_dim)))          # :191-198
                    self.eps.append(GINEps(0.0))                                                   # :199
                else:
                    self.convs.append(GCNConv(hidden_input_dim, hidden_dim, aggr="add"))           # :200-201
            else:
                raise NotImplementedError(
                    f"--neigh_conv_type {args.conv_type}: only SAGE (SHMP; homogeneous in ablation_gnns.py), GIN and GCN "
                    "(homogeneous, ablation_gnns.py) and --gossip_conv_type GOSSIP are on the hot path; GAT and PNACONV "
                    "are not")
        self.post_input_dim = hidden_dim * args.layer_num + pre_dim_out          # :207
        self.node_types: Optional[List[str]] = None
        self.edge_types: Optional[List[Tuple[str, str, str]]] = None
        # the row types a HOMOGENEOUS core packs operands for (row_types()); the owner narrows it to what its batches
        # hold (NeighborhoodCountingModel: count + canonical for the target model, union_node for the query model)
        self.homo_row_types: List[str] = list(HOMO_ROW_TYPES)

    def to_hetero(self, node_types: Sequence[str], edge_types: Sequence[Tuple[str, str, str]]):
        """pyg.nn.to_hetero(aggr="sum") equivalent for this module [EXT, SURVEY App. C]."""
        if self.conv_type in PLAIN_CONV_TYPES:
            raise NotImplementedError(f"--neigh_conv_type {self.conv_type}: to_hetero of a GIN / GCN core is not on the "
                                      "hot path; these cores run homogeneous (use_hetero=False, ablation_gnns.py)")
        if self.conv_type != "SAGE":
            raise NotImplementedError("to_hetero is only defined for the SAGE (SHMP) core")
        if self.node_types is not None:
            raise RuntimeError("model is already heterogeneous")
        in_dim = self.pre_mp[0].in_features
        hd = self.hidden_dim
        self.pre_mp = nn.Sequential(nn.ModuleDict({t: nn.Linear(in_dim, hd) for t in node_types}))
        self.convs = nn.ModuleList([
            nn.ModuleDict({"__".join(et): SAGEConv(hd, hd) for et in edge_types})
            for _ in range(self.layer_num)])
        self.updates = nn.ModuleList([
            nn.ModuleDict({t: nn.Linear(2 * hd, hd) for t in node_types})
            for _ in range(self.layer_num)])
        self.node_types, self.edge_types = list(node_types), [tuple(e) for e in edge_types]
        return self

    # ---- per-type / per-relation accessors ----------------------------------------------------------------------------
    # What the weight packers read.  After ``to_hetero`` they index the per-type / per-relation ModuleDicts; a
    # HOMOGENEOUS core (use_hetero=False, never converted: the reference's ablation_gnns.py model) has ONE pre_mp, one
    # convs[l].lin and one updates[l], which every row type and relation slot reads -- so the same Parameter enters a
    # fold several times and autograd sums its gradient over the uses.  (Aliasing the module inside ModuleDicts would
    # duplicate the state-dict keys.)
    def is_homogeneous(self) -> bool:
        return self.node_types is None and not self.use_hetero and (self.conv_type == "SAGE" or self.is_plain())

    def is_plain(self) -> bool:
        """a GIN or GCN core: homogeneous, run by the plain-layer kernel at every width (plain_forward)"""
        return self.conv_type in PLAIN_CONV_TYPES

    def row_types(self) -> List[str]:
        """the row types a batch can hold: the model's node types, or ``homo_row_types`` for a homogeneous core"""
        if self.node_types is not None:
            return self.node_types
        if not self.is_homogeneous():
            raise NotImplementedError("the SAGE core has no node types yet: call to_hetero_old()/to_hetero() first "
                                      "(main.py:221-224), or build the model with use_hetero=False (ablation_gnns.py)")
        return self.homo_row_types

    def pre_lin(self, t: str) -> nn.Linear:
        return self.pre_mp[0] if self.node_types is None else self.pre_mp[0][t]

    def conv(self, l: int, key: str) -> SAGEConv:
        return self.convs[l] if self.node_types is None else self.convs[l][key]

    def update(self, l: int, t: str) -> nn.Linear:
        return self.updates[l] if self.node_types is None else self.updates[l][t]

    def slot_keys(self, dst_type: str) -> List[str]:
        """Module keys of the relation slots (triangle, tride) x (source types) feeding dst_type."""
        if self.node_types is None:
            self.row_types()                     # (raises unless homogeneous)
            return [HOMO_KEY] * (4 if dst_type == "count" else 2)      # one relation: one weight, one bias
        keys = []
        srcs = [dst_type] if len(self.node_types) == 1 else ["count", "canonical"]
        for src in srcs:
            if src == "canonical" and dst_type == "canonical":
                continue
            for rel in ("union_triangle", "union_tride"):
                et = (src, rel, dst_type)
                if et in self.edge_types:
                    keys.append("__".join(et))
                elif (src, "union", dst_type) in self.edge_types:   # use_tconv=False: one weight
                    keys.append("__".join((src, "union", dst_type)))
                else:
                    raise KeyError(f"edge type {et} not in model metadata")
        return keys

    def forward(self, x, edge_index, query_emb=None):
        """``BaseGNNCore.forward(x, edge_index, query_emb=None)`` with the reference's arguments and return value
        (gnn_model.py:230-277): pre_mp, then per layer conv -> (SAGE: updates[i](cat(x_neigh, x))) -> relu -> dropout
        -> running cat, op by op on this library's kernels (the stand-alone ``SAGEConv.forward`` /
        ``GossipConv.forward`` + ``ops.gemm``).  Inference only (no autograd); ``BaseGNN.forward`` -- what the models
        call -- runs the same layers as fused kernels on the canonical-partition batches.

        SAGE after ``to_hetero``: ``x`` = {node type: [n_t, input_dim]}, ``edge_index`` = {(src, rel, dst): [2, E]} with
        indices local to their node types; returns {node type: [n_t, 64 (L + 1)]}; the relations into one destination
        type are summed pairwise in metadata order (pyg.nn.to_hetero(aggr="sum")).  GOSSIP: ``x`` [N, input_dim],
        ``edge_index`` [2, E], ``query_emb`` [1, 64] of ONE query; returns [N, 64 (L + 2)]."""
        from collections import deque
        with torch.no_grad():
            if self.conv_type == "GOSSIP":
                dev = x.device
                lin = self.pre_mp[0]
                h = ops.linear_smallk(x.float().contiguous(), ops.transposed(lin.weight), lin.bias)       # :231
                if self.input_pattern_emb:                                                                # :233-240
                    if query_emb is None:
                        raise AssertionError("query_emb is required (input_pattern_emb)")
                    h = torch.cat((query_emb.reshape(1, -1).float().to(dev).expand(h.shape[0], -1), h), dim=-1)
                ei = edge_index[:, edge_index[0] != edge_index[1]] if edge_index.numel() else edge_index  # :246
                ei = torch.unique(torch.cat([ei, ei.flip(0)], 1), dim=1) if ei.numel() else ei            # :247
                ew = ei[0] < ei[1]                                                                        # :248
                emb = h
                for l, conv in enumerate(self.convs):
                    h = conv(h.contiguous(), ei, edge_weight=ew, query_emb=query_emb)                     # :257-260
                    h = self._relu_dropout(h, l)                                                          # :273-274
                    emb = torch.cat((emb, h), 1)                                                          # :275
                return emb
            if self.node_types is None:
                # homogeneous SAGE (ablation_gnns.py): ``x`` [N, input_dim], ``edge_index`` [2, E]; returns [N, 64 (L + 1)]
                self.row_types()                                                                          # (raises unless homogeneous)
                if self.is_plain():
                    return self._forward_plain(x, edge_index)
                lin = self.pre_mp[0]
                h = ops.linear_smallk(x.float().contiguous(), ops.transposed(lin.weight), lin.bias)       # :231
                emb = h
                for l in range(self.layer_num):
                    x_neigh = self.convs[l](h, edge_index)                                                # :262
                    up = self.updates[l]
                    h = self._relu_dropout(ops.gemm(x_neigh, ops.transposed(up.weight), up.bias, a2=h.contiguous()), l)
                    emb = torch.cat((emb, h), 1)                                                          # :275
                return emb
            xs ={t: ops.linear_smallk(x[t].float().contiguous(), ops.transposed(self.pre_mp[0][t].weight),
                                       self.pre_mp[0][t].bias) for t in self.node_types}
            emb = dict(xs)
            for l in range(self.layer_num):
                outs = {t: deque() for t in self.node_types}
                for (s, r, d) in self.edge_types:
                    ei = edge_index.get((s, r, d))
                    outs[d].append(self.convs[l]["__".join((s, r, d))]((xs[s], xs[d]), ei))               # :262
                new = {}
                for t in self.node_types:
                    q = outs[t]
                    while len(q) >= 2:                      # to_hetero's pairwise sum over a common destination
                        q.append(q.popleft() + q.popleft())
                    up = self.updates[l][t]
                    hcat = ops.gemm(q[0], ops.transposed(up.weight), up.bias, a2=xs[t].contiguous())      # :264
                    new[t] = self._relu_dropout(hcat, l, t)
                xs = new
                emb = {t: torch.cat((emb[t], xs[t]), dim=1) for t in self.node_types}
            return emb

    def _forward_plain(self, x, edge_index):
        """the GIN / GCN branches of ``forward`` (gnn_model.py:262-270), op by op on rows zero-padded to the padded
        width: GIN  x = relu(updates[l](agg + (1 + eps_l x)))  -- the parentheses as the reference writes them;
        GCN  x = relu(convs[l](x)).  Returns [N, hidden (L + 1)]."""
        hd, wp = self.hidden_dim, padded_width(self.hidden_dim)
        lin = self.pre_mp[0]
        h = ops.linear_smallk(x.float().contiguous(), _pad_to(lin.weight.t(), lin.in_features, wp).contiguous(),
                              _pad_to(lin.bias, wp).contiguous())                                         # :231
        live = torch.zeros(wp, device=h.device)
        live[:hd] = 1.0                                          # the constant 1 reaches the true channels only
        emb = [h]
        for l in range(self.layer_num):
            agg = _plain_aggregate(h, edge_index, h.shape[0])                                             # :262
            if self.conv_type == "GIN":
                u = self.updates[l]
                z = agg + (live + self.eps[l]() * h)                                                      # :266
                t = ops.gemm(z.contiguous(), _pad_to(u[0].weight.t(), wp, wp).contiguous(), _pad_to(u[0].bias, wp).contiguous(),
                             act=ops.ACT_RELU)
                h = ops.gemm(t, _pad_to(u[2].weight.t(), wp, wp).contiguous(), _pad_to(u[2].bias, wp).contiguous())
            else:
                c = self.convs[l]
                h = ops.gemm(agg, _pad_to(c.lin.weight.t(), wp, wp).contiguous(), _pad_to(c.bias, wp).contiguous())  # :268-270
            h = self._relu_dropout(h, l)                                                                  # :273-274
            emb.append(h)
        return torch.cat([e[:, :hd] for e in emb], 1)                                                     # :275

    def _relu_dropout(self, h, layer, node_type=None):
        """relu (gnn_model.py:273) and, in training mode with dropout > 0, F.dropout (:274) as this library's
        counter-based factor (ops.dropout_mask) -- one key per call, the site id separates layers / node types."""
        h = torch.relu(h)
        p = float(self.dropout or 0.0)
        if self.training and p > 0.0 and h.numel():
            site = 16 * layer + (0 if node_type is None else 1 + self.node_types.index(node_type))
            h = h * ops.dropout_mask(ops.DropSite(ops.rng_next(h.device), site % 256, p), h.shape[0], h.shape[1])
        return h


class BaseGNN(nn.Module):
    """core + anchor MLP + pool + post MLP (gnn_model.py:18-112)."""

    def __init__(self, input_dim, hidden_dim, output_dim, args, **kwargs):
        super().__init__()
        self.dropout = args.dropout
        self.layer_num = args.layer_num
        self.conv_type = args.conv_type
        self.use_hetero = args.use_hetero
        self.args, self.kwargs = args, kwargs
        self.output_dim = output_dim
        self.gnn_core = BaseGNNCore(input_dim, hidden_dim, output_dim, args, **kwargs)
        p = self.gnn_core.post_input_dim
        self.anchor_mlp = nn.Sequential(nn.Linear(p, p), nn.LeakyReLU(0.1))              # :40-42
        self.post_mp = nn.Sequential(                                                    # :44-53
            nn.Linear(p, hidden_dim), nn.Dropout(args.dropout), nn.LeakyReLU(0.1),
            nn.Linear(hidden_dim, hidden_dim), nn.ReLU(),
            nn.Linear(hidden_dim, 256), nn.ReLU(),
            nn.Linear(256, output_dim))
        self._pack_cache = None

    # -- weight folding ---------------------------------------------------------------------------
    def _param_version(self):
        # (buffers too: GIN's eps enters the packed operands and the cached query embeddings)
        return tuple((p.data_ptr(), p._version) for p in list(self.parameters()) + list(self.buffers()))

    def packed(self):
        """Kernel operands folded from the parameters; cached until a parameter changes."""
        ver = self._param_version()
        if self._pack_cache is None or self._pack_cache[0] != ver:
            with torch.no_grad():
                pk = pack_gossip(self) if self.conv_type == "GOSSIP" else \
                    (pack_plain(self) if self.gnn_core.is_plain() else
                     (pack_shmp_wide(self) if self.is_wide() else pack_shmp(self)))
            self._pack_cache = (ver, pk)
        return self._pack_cache[1]

    def forward(self, data, query_emb=None, drop_key=None):
        if self.conv_type == "GOSSIP":
            if not isinstance(data, GossipBatch):
                raise TypeError("gossip BaseGNN.forward expects a desco_amd.batch.GossipBatch")
            if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
                return gossip_forward_train(self, data, query_emb)
            return gossip_forward(self, data, query_emb)
        if not isinstance(data, (NeighborhoodBatch, QueryBatch, GraphBatch)):
            raise TypeError("BaseGNN.forward expects a NeighborhoodBatch, QueryBatch or GraphBatch")
        # a homogeneous model (use_hetero=False: ablation_gnns.py) runs the same fused path on its one set of weights
        # (BaseGNNCore accessors); a hetero model that has not been converted yet is refused here
        self.gnn_core.row_types()
        if self.gnn_core.is_homogeneous() and isinstance(data, NeighborhoodBatch) and data.node_feature is None:
            raise ValueError("a homogeneous model marks the anchor by node_feature (1 on canonical rows, 0 elsewhere): "
                             "this NeighborhoodBatch carries none (NeighborhoodDataset(hetero_graph=False) builds it)")
        if self.is_wide():
            # (the padded channels are exactly zero: callers see the true width)
            return self.forward_padded(data, drop_key)[:, :self.output_dim]
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return shmp_forward_train(self, data, drop_key)
        return shmp_forward(self, data)

    def forward_classes(self, data):
        """``forward`` at inference for callers whose own work is row-local (the count head): ``(emb, rows)`` with ``rows``
        None and ``emb`` = ``forward(data)``, or (POOL_CLASS_TABLE) ``emb`` one row per pooling class and ``forward(data)`` =
        ``emb[rows]``, which is then never formed"""
        train = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if self.conv_type == "GOSSIP" or not isinstance(data, NeighborhoodBatch) or self.is_wide() or train:
            return self(data), None
        self.gnn_core.row_types()                # (a hetero model that has not been converted yet is refused, as in forward)
        if self.gnn_core.is_homogeneous():
            return self(data), None
        return shmp_forward_classes(self, data)

    def is_wide(self) -> bool:
        """True for a SAGE model of another width than 64 (it runs the wide path, shmp_forward_wide) and for a plain GIN /
        GCN model of ANY width (plain_forward): both work on operands zero-padded to padded_width(hidden_dim)"""
        return self.conv_type != "GOSSIP" and (self.gnn_core.hidden_dim != H or self.gnn_core.is_plain())

    def forward_padded(self, data, drop_key=None) -> torch.Tensor:
        """wide path: the graph embeddings [B, padded_width(output_dim)] (zero beyond output_dim)"""
        train = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if self.gnn_core.is_plain():
            return plain_forward_train(self, data, drop_key) if train else plain_forward(self, data)
        if train:
            return shmp_forward_train_wide(self, data, drop_key)
        return shmp_forward_wide(self, data)


# -------------------------------------------------------------------------------------------------
# SHMP (neighborhood / query) path
# -------------------------------------------------------------------------------------------------
def _mv(A: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """A [..., m, k] times v [..., k] -> [..., m] as a broadcast product and a row sum.  torch routes a matrix-vector
    product to rocBLAS gemv, whose split reduction uses float atomics: the folded weights -- and with them a seeded
    training run -- were not reproducible from run to run.  This form is a fixed-order reduction."""
    return (A * v.unsqueeze(-2)).sum(-1)


def _vm(v: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """v [k] times A [k, n] -> [n], same reason as ``_mv``."""
    return (v.unsqueeze(-1) * A).sum(0)


def _lin_t(lin: nn.Linear):
    return lin.weight.t().contiguous(), lin.bias.contiguous()


def pack_shmp(gnn: BaseGNN, bf16_planes: bool = True) -> dict:
    """bf16_planes: also emit the pre-split weight planes of the bf16x6 GEMMs (inference only)."""
    core = gnn.gnn_core
    pk = {"pre": {}, "layers": []}
    for t in core.row_types():
        pk["pre"][t] = _lin_t(core.pre_lin(t))
    # Folding (U_n W_s)^T for every (layer, destination type, slot) and U_n sum_s b_s + c for every
    # (layer, type): two batched matmuls instead of ~100 tiny ones (the training step re-folds the
    # weights every step; per-product launches made it host-bound).  Differentiable.
    items, un_items, bias_items, un_rows = [], [], [], []
    for l in range(core.layer_num):
        for t in core.row_types():
            Un = core.update(l, t).weight[:, :H]
            bsum, seen = 0, set()
            for key in core.slot_keys(t):
                conv = core.conv(l, key)
                items.append(conv.lin.weight)
                un_items.append(Un)
                if key not in seen:      # one bias per edge TYPE (use_tconv=False ties two slots)
                    bsum = bsum + conv.lin.bias
                    seen.add(key)
            bias_items.append(bsum)
            un_rows.append(Un)
    folded = torch.bmm(torch.stack(un_items), torch.stack(items)).transpose(1, 2)    # (U_n W_s)^T
    fbias = _mv(torch.stack(un_rows), torch.stack(bias_items))
    it = ib = 0
    for l in range(core.layer_num):
        per_type = {}
        for t in core.row_types():
            U, c = core.update(l, t).weight, core.update(l, t).bias
            Ux = U[:, H:]
            nslots = len(core.slot_keys(t))
            blocks = [folded[it + k] for k in range(nslots)]
            it += nslots
            blocks.append(Ux.t())
            fb = fbias[ib] + c
            ib += 1
            entry = {"wt": torch.cat(blocks, 0).contiguous(), "b": fb.contiguous()}
            if len(blocks) == 5:
                # count destinations: the two canonical->count relations have at most one source
                # per row; apply them from a pre-transformed table (K 320 -> 192)
                entry["wt_mfma"] = torch.cat([blocks[0], blocks[1], blocks[4]], 0).contiguous()
                entry["wt_tab"] = torch.cat([blocks[2], blocks[3]], 1).contiguous()      # [64,128]
                if bf16_planes and GEMM_BF16X6:
                    entry["wt_tab_l64"] = ops.linear64_planes(entry["wt_tab"].t())     # [2,3,64,64]
            if bf16_planes and SHMP_BF16X6:
                # n-major operand planes of the MFMA blocks of the fused layer (K <= 192): fp16 (hi, lo) + one scale
                # per matrix, or bf16 (hi, mid, lo)
                split = ops.split_f16_planes if SHMP_F16X3 else ops.split_bf16_planes
                for name in ("wt_mfma", "wt"):
                    if name in entry and entry[name].shape[0] <= 192:
                        entry[name + "_x6"] = split(entry[name].t())
            per_type[t] = entry
        pk["layers"].append(per_type)
    pk["anchor"] = _lin_t(gnn.anchor_mlp[0])
    pk["post"] = [_lin_t(gnn.post_mp[i]) for i in (0, 3, 5, 7)]
    if not (bf16_planes and GEMM_BF16X6):
        return pk
    # n-major ([out, in]) pre-split operands of the bf16x6 GEMM
    _split = ops.split_f16_planes if GEMM_F16X3 else ops.split_bf16_planes
    pk["anchor_nk"] = (_split(gnn.anchor_mlp[0].weight), gnn.anchor_mlp[0].bias.contiguous())
    # (64-input layers run on the streaming row-wise kernel: planes per 64-column output block)
    pk["post_nk"] = [((ops.linear64_planes(gnn.post_mp[i].weight) if gnn.post_mp[i].in_features == 64
                       else ops.split_bf16_planes(gnn.post_mp[i].weight)),
                      gnn.post_mp[i].bias.contiguous()) for i in (0, 3, 5, 7)]
    # post_mp.3 -> .5 -> .7 in one launch (ops.post_mp_tail): the three matrices as fp16 (hi, lo) planes
    dims = [tuple(gnn.post_mp[i].weight.shape) for i in (3, 5, 7)]
    if POST_TAIL_FUSED and GEMM_F16X3 and dims == [(64, 64), (256, 64), (64, 256)]:
        pk["post_tail"] = [v for i in (3, 5, 7)
                           for v in (ops.split_f16_planes(gnn.post_mp[i].weight), gnn.post_mp[i].bias.contiguous())]
    return pk


# post_mp.3 -> .5 -> .7 in one launch (desco_post_mp_tail_f16x3_f32): the [B, 64] and [B, 256] intermediates never reach HBM
POST_TAIL_FUSED = os.environ.get("DESCO_POST_TAIL_FUSED", "1") != "0"


class _PostMp0(object):
    """post_mp.0's output computed by _shmp_pooled itself (the pooled operand never materialised).  ``rows``: None, or
    (POOL_CLASS_TABLE) ``h0`` holds one row per pooling class and neighborhood b's row is ``h0[rows[b]]`` ([B] int32)"""
    __slots__ = ("h0", "rows")

    def __init__(self, h0, rows=None):
        self.h0, self.rows = h0, rows


def _post_mp(pk, pooled):
    if GEMM_BF16X6 and "post_nk" in pk:
        def lin(a, w, b, act=ops.ACT_NONE, slope=0.0):
            f = ops.linear64 if w.dim() == 4 else ops.gemm_split
            return f(a, w, b, act=act, slope=slope)
        (w0, b0), (w3, b3), (w5, b5), (w7, b7) = pk["post_nk"]
        h = pooled.h0 if isinstance(pooled, _PostMp0) else lin(pooled, w0, b0, ops.ACT_LEAKY, 0.1)
        if POST_TAIL_FUSED and "post_tail" in pk:
            return ops.post_mp_tail(h, *pk["post_tail"])
        h = lin(h, w3, b3, ops.ACT_RELU)
        h = lin(h, w5, b5, ops.ACT_RELU)
        return lin(h, w7, b7)
    (w0, b0), (w3, b3), (w5, b5), (w7, b7) = pk["post"]
    h = ops.gemm(pooled, w0, b0, act=ops.ACT_LEAKY, slope=0.1)
    h = ops.gemm(h, w3, b3, act=ops.ACT_RELU)
    h = ops.gemm(h, w5, b5, act=ops.ACT_RELU)
    return ops.gemm(h, w7, b7)


def _gemm_planes(a, w, b, **kw):
    """A GEMM on pre-split weight planes: f16x3 (ops.F16Planes) or bf16x6 (int16 [3, n, k])."""
    return (ops.gemm_f16x3 if isinstance(w, ops.F16Planes) else ops.gemm_split)(a, w, b, **kw)


def _first_layer_coef(pk, t, su, S, x0, src_of_slot, dev):
    """[S+1, 64] coefficients of the closed-form first layer for destination type ``t`` (folded once per
    weight version): rows s < su = x0_src(s) W_s, unused slots zero, last row = x0_t W_self + bias."""
    ck = ("layer0_coef", t, S)
    if ck not in pk:
        e = pk["layers"][0][t]
        wt = e["wt"]                                    # [(su+1)*64, 64]
        rows = [_vm(x0[src_of_slot(t, s)], wt[s * H:(s + 1) * H]) for s in range(su)]
        rows += [torch.zeros(H, device=dev)] * (S - su)  # unused slots of this type
        rows.append(_vm(x0[t], wt[su * H:(su + 1) * H]) + e["b"])
        pk[ck] = torch.stack(rows).contiguous()
    return pk[ck]


def _anchor_const_input_weights(pk, gnn):
    """anchor_mlp's weight planes without the first 64 columns and its bias with their product folded in (once per
    weight version)"""
    if "anchor_nk_const" not in pk:
        w, b = gnn.anchor_mlp[0].weight, gnn.anchor_mlp[0].bias
        x0 = pk["pre"]["canonical"][1]
        _split = ops.split_f16_planes if GEMM_F16X3 else ops.split_bf16_planes
        pk["anchor_nk_const"] = (_split(w[:, H:].contiguous()), (b + _mv(w[:, :H], x0)).contiguous())


def _anchor_const_input(pk, gnn, canon, row_bound=None):
    """anchor_mlp (gnn_model.py:69-73) on emb["canonical"] when the input layer is constant (all-zero node
    features: x^0 of every canonical row is pre_mp's bias): the first 64-column block of the operand is the
    same row for every neighborhood, so its product is folded into the bias and the GEMM runs with
    K = 512 instead of 576 (one ninth of the largest dense product of the pass)."""
    _anchor_const_input_weights(pk, gnn)
    kw = {"row_scale": row_bound} if (row_bound is not None and isinstance(pk["anchor_nk_const"][0], ops.F16Planes)) else {}
    return _gemm_planes(canon[:, H:], *pk["anchor_nk_const"], act=ops.ACT_LEAKY, slope=0.1, **kw)


# The trunk on tables of distinct rows.  Under ZeroNodeFeat the count rows of X_k are a function of far fewer
# things than there are rows -- a molecule batch has a few thousand to a few ten thousand distinct ones per layer for millions
# of rows (COX2-shaped: 531 of X_1, 1 427 of X_2, 12 316 of X_3, 28 561 of X_4, 37 756 of X_8; the classes stop growing) -- so
# _shmp_pooled keeps X_k's count rows as a table of the distinct rows, table k, and a class per row.  Every path below is
# bit-identical to the launches on the materialised tensors (the layer kernels' arithmetic is row-local, the sums keep their
# order), has its own switch, and stacks on the one before it; the tests flip the switches to get the earlier launches back.
#
# Level 1: X_1 is the closed-form first layer, a function of a row's four slot degrees (NeighborhoodBatch.degree_table_index).
# X_1's count rows are never written: the second layer gathers from table 1 and recomputes its own rows from their degrees
# (desco_shmp_layer_pool_table_f16x3_f32)
FIRST_LAYER_TABLE = os.environ.get("DESCO_FIRST_LAYER_TABLE", "1") != "0"

# The table slots: a block without an entry in one of the two (molecule graphs: table slot 0, the canonical->count TRIANGLE
# relation) gets no table columns for it -- the canonical->count product writes [B, 64] instead of [B, 128], the count launches
# read the narrow table (desco_shmp_layer_narrow_f16x3_f32, NeighborhoodBatch.table_empty) -- and the second layer's product
# runs on the DISTINCT first-layer canonical rows only (NeighborhoodBatch.canonical_table_index)
TABLE_NARROW = os.environ.get("DESCO_TABLE_NARROW", "1") != "0"

# Level k >= 2, one recurrence (NeighborhoodBatch.layer2_table_index, layer3_table_index, deep_table_index): a count row of X_k
# is a function of its own row of X_{k-1} and, per CSR entry in order, of the source's row of X_{k-1} -- at k = 2 of its slot
# degrees and its segment of first-layer table ids.  Layer k's count launch runs on one representative per class, sources and
# own rows in table k - 1 (own rows from their degrees at k = 2; desco_shmp_layer_selfidx_f16x3_f32 above that), the table
# product on the distinct canonical rows of X_{k-1} only, and leaves table k.  Behind the deepest level's launch one walk over
# the count rows leaves the pooled partial sums of every table layer (ops.table_rows_pool: desco_table_rows_pool_f32 for one
# table, desco_table_rows_pool2_f32 for two, desco_table_rows_pool3_f32 / desco_table_rows_pooln_f32 for more).  Layer K + 1,
# if the model has one, gathers from table K with the column ids of that level's ``vcol_k``, its own rows through the classes.
# Level 2, where both first-layer tables exist: the walk writes the rows of X_2 as well
SECOND_LAYER_TABLE = os.environ.get("DESCO_SECOND_LAYER_TABLE", "1") != "0"

# ... unless X_2's count rows are never written either -- the third layer's two launches gather from table 2 and the walk
# leaves the partial sums alone; models of three layers or more, blocks of at least NeighborhoodBatch.LAYER2_GATHER_MIN_ROWS
# count rows
SECOND_LAYER_GATHER = os.environ.get("DESCO_SECOND_LAYER_GATHER", "1") != "0"

# The first layer's pooled partial sums from the same walk, both tables staged in LDS -- the first layer's own pooled launch
# (desco_degree_affine_pool_f32 with out = NULL: the affine map evaluated per row for rows that are table1[row_id]) is then
# not issued; blocks of at least NeighborhoodBatch.POOL_TABLES_MIN_ROWS count rows
POOL_TABLES = os.environ.get("DESCO_POOL_TABLES", "1") != "0"

# Level 3: X_3's count rows are never written, the fourth layer gathers from table 3, and the walk -- now of three tables --
# follows this level's launch.  Where SECOND_LAYER_GATHER is active and the batch has the index (blocks of at least
# NeighborhoodBatch.LAYER3_MIN_ROWS count rows)
THIRD_LAYER_TABLE = os.environ.get("DESCO_THIRD_LAYER_TABLE", "1") != "0"

# Levels 4 .. K: the same for every further layer with a class index.  Where THIRD_LAYER_TABLE is active and the batch has the
# index (blocks of at least NeighborhoodBatch.DEEP_TABLE_MIN_ROWS count rows)
DEEP_LAYER_TABLES = os.environ.get("DESCO_DEEP_LAYER_TABLES", "1") != "0"

# a table level as _shmp_pooled reads it, the layout of layer3_table_index and deep_table_index (level 2 has no ``rep_self`` and
# no canonical classes: its own rows come from the degrees, its table product from canonical_table_index)
_TableLevel = namedtuple("_TableLevel", "cls rep_uptr rep_vcol rep_self vcol ccls crep")


def _layer2_table(canon_uptr: torch.Tensor, S: int, coef: torch.Tensor, planes: torch.Tensor) -> torch.Tensor:
    """the second layer's canonical->count table on the U_c distinct first-layer canonical rows: the closed-form first layer on
    the distinct degree tuples (``canon_uptr`` of canonical_table_index, ``coef`` the canonical rows' coefficients), then the
    row-wise table product -- row u equals the full product's row of every canonical row with tuple u, bit for bit"""
    rows = torch.empty(((canon_uptr.numel() - 1) // S, H), device=canon_uptr.device)
    ops.degree_affine(canon_uptr, 0, rows.shape[0], S, coef, ops.ACT_RELU, 0.0, rows)
    return ops.linear64(rows, planes)


# the pooled embeddings [B, 64 (L + 1)] are never written: post_mp.0 forms its operand's chunks from the anchor rows and
# the fused pooling's partial sums in its load phase (desco_pool_post_bf16x6_f32; neighborhoods of at most 33 count rows)
POOL_POST_FUSED = os.environ.get("DESCO_POOL_POST_FUSED", "1") != "0"

# ... and with the anchor MLP in the same launch (desco_anchor_pool_post_f16x3_f32): the anchor rows [B, 64 (L + 1)] are
# never written either (f16x3 anchor on the producer-written row bound, first block folded, L in {2, 5, 8})
ANCHOR_POST_FUSED = os.environ.get("DESCO_ANCHOR_POST_FUSED", "1") != "0"

# ... unless the anchor operands are a table too: where the table levels reach the last layer, the canonical rows' classes of
# X_L (NeighborhoodBatch.anchor_class_index: COX2-shaped x64 has a few thousand for 1.2 M neighborhoods) determine the whole
# anchor operand [X_1 | ... | X_L] and its row bound, so the anchor MLP runs on one representative per class -- a gather and a
# U_a-row f16x3 GEMM -- and post_mp.0 reads its rows through the classes (desco_pool_post_rows_bf16x6_f32).  Taken exactly
# where the fused launch above would be, on blocks of at least NeighborhoodBatch.ANCHOR_CLASS_MIN_ROWS neighborhoods; off
# wherever DEEP_LAYER_TABLES is off
ANCHOR_CLASS_TABLE = os.environ.get("DESCO_ANCHOR_CLASS_TABLE", "1") != "0"

# ... and the canonical rows themselves: X_l's canonical rows exist as a table of their distinct rows per level only
# (NeighborhoodBatch.canonical_class_tables), written by the closed-form first layer on the distinct degree tuples and by the
# canonical launches on one representative per class -- sources in the count rows' table, own rows gathered from the table
# before --; the table products read them as they are, the anchor operand's U_a rows are gathered from them, and neither the
# [B, 64 (L + 1)] operand nor its [B] row bound is allocated.  Where ANCHOR_CLASS_TABLE is taken
CANON_CLASS_TABLES = os.environ.get("DESCO_CANON_CLASS_TABLES", "1") != "0"


# ... and everything behind the trunk: where ANCHOR_CLASS_TABLE is taken, a neighborhood's row of post_mp.0's operand is a
# function of its anchor class, of where the pooling's 16-row tile cuts fall inside it and of the ordered top-level classes of
# its count rows (NeighborhoodBatch.pool_class_index: COX2-shaped x64 has 52 k such classes for 1.2 M neighborhoods), and the
# rest of the model is row-local.  The pooled sums are formed on one representative per class (desco_class_rows_pool_f32, in
# place of the walk over all count rows, in the walk's order of additions), post_mp and the count head run on those rows, and
# the counts are handed out to the neighborhoods by one gather (desco_gather_rows_f32).  Blocks of at least
# NeighborhoodBatch.POOL_CLASS_MIN_ROWS neighborhoods
POOL_CLASS_TABLE = os.environ.get("DESCO_POOL_CLASS_TABLE", "1") != "0"


def shmp_forward(gnn: BaseGNN, batch) -> torch.Tensor:
    """BaseGNN.forward, hetero path (gnn_model.py:58-109) -> graph embeddings [B, 64]."""
    emb, rows = shmp_forward_classes(gnn, batch)
    return emb if rows is None else ops.gather_rows(emb, rows)


def shmp_forward_classes(gnn: BaseGNN, batch):
    """``shmp_forward`` with the embeddings as the pass leaves them: ``(emb, rows)``, ``rows`` None and ``emb`` [B, 64], or
    (POOL_CLASS_TABLE) ``emb`` one row per pooling class and neighborhood b's embedding ``emb[rows[b]]`` -- for callers whose
    own work is row-local too (the count head)"""
    pooled = _shmp_pooled(gnn, batch, fuse_post0=True)
    return _post_mp(gnn.packed(), pooled), (pooled.rows if isinstance(pooled, _PostMp0) else None)          # :108


def _shmp_pooled(gnn: BaseGNN, batch, fuse_post0: bool = False):
    """The pooled embeddings [B, 64 (L+1)] of BaseGNN.forward before post_mp (gnn_model.py:58-107)."""
    pk = gnn.packed()
    core = gnn.gnn_core
    L = core.layer_num
    dev = batch.vrowptr.device
    N, S, B = batch.num_rows, batch.slots, batch.num_graphs
    P = H * (L + 1)
    nb = isinstance(batch, NeighborhoodBatch)
    if nb:
        Nc = batch.num_count
        groups = [("count", 0, Nc, 4), ("canonical", Nc, N, 2)]
    else:
        Nc = N
        groups = [("union_node", 0, N, 2)]
    f16 = GEMM_BF16X6 and GEMM_F16X3 and SHMP_BF16X6 and SHMP_F16X3
    # ZeroNodeFeat (workload.py:431-440): pre_mp(x) is its bias, identical for every node of a type, so X_0 is never
    # materialised and layer 0 is a degree-affine map (desco_hip.h)
    const_input = batch.node_feature is None and L >= 1
    # fused pooling: the count launches leave partial neighborhood sums, reduced after the anchor MLP
    fpool = SHMP_BF16X6 and GEMM_BF16X6 and nb and Nc > 0
    # canonical rows only in the anchor operand: the f16x3 fused path with its direct column-block writes
    canon_once = CANON_ROWS_ONCE and const_input and nb and f16 and N > Nc > 0
    # the count rows' first-layer launch leaves their pooled partial sums like the fused layers' launches do (round 6:
    # saves the one read of X_1 that its segment sum cost)
    pool1 = POOL_FIRST_LAYER and const_input and fpool
    # ... and with the table form of the second layer's launches they are not stored either (tab1: the table index)
    tab1 = None
    if (FIRST_LAYER_TABLE and pool1 and canon_once and L >= 2 and "wt_tab" in pk["layers"][1]["count"]
            and isinstance(pk["layers"][1]["count"].get("wt_mfma_x6"), ops.F16Planes)):
        tab1 = batch.degree_table_index()
    # no table columns for an empty table slot 1; then also layer 2's table from the distinct canonical degree tuples
    temp = batch.table_empty if (TABLE_NARROW and nb and f16 and Nc > 0) else 0      # (bit t: table slot t is empty)
    tblock = 1 if temp == 1 else 0                                                  # the 64-row block of wt_tab_l64 still needed
    ctab = batch.canonical_table_index() if (temp and tab1 is not None) else None
    # lev[k]: the class index of table level k = 2 .. K -- layer k's count launch runs on the distinct rows of its OUTPUT -- and
    # tbl[k], k = 1 .. K: the table of X_k's distinct count rows.  Levels stack: each needs the one below and its own switch
    lev, tbl = {}, {}
    fp16_form = lambda e: ("wt_tab" in e["count"] and isinstance(e["count"].get("wt_mfma_x6"), ops.F16Planes)
                           and isinstance(e["canonical"].get("wt_x6"), ops.F16Planes))
    if SECOND_LAYER_TABLE and ctab is not None and fpool and L >= 2:
        t2 = batch.layer2_table_index()                          # (None: the batch is not eligible)
        if t2 is not None:
            lev[2] = _TableLevel(t2[0], t2[1], t2[2], None, t2[3], None, None)
    # gather2: table 2 is all there is of X_2's count rows, the third layer's launches gather from it (the fp16 forms of both
    # node types, so that no launch of layers 2 and 3 reads or writes a row of X_2); otherwise the level-2 walk writes X_2
    gather2 = False
    if SECOND_LAYER_GATHER and 2 in lev and L >= 3 and Nc >= batch.LAYER2_GATHER_MIN_ROWS:
        l1, l2 = pk["layers"][1], pk["layers"][2]
        gather2 = fp16_form(l2) and all(isinstance(l1[t].get(k), ops.F16Planes) for t, k in (("count", "wt_mfma_x6"),
                                                                                           ("canonical", "wt_x6")))
    if THIRD_LAYER_TABLE and gather2 and (L < 4 or fp16_form(pk["layers"][3])):
        t3 = batch.layer3_table_index()
        if t3 is not None:
            lev[3] = _TableLevel(*t3)
    if DEEP_LAYER_TABLES and 3 in lev and L >= 4:
        for k, tk in enumerate(batch.deep_table_index(), 4):
            if k > L or (k < L and not fp16_form(pk["layers"][k])):    # (layer k, if any, gathers from table k)
                break
            lev[k] = _TableLevel(*tk)
    # X_k's count rows exist as table k only (never allocated, never written): every level but a second without gather2
    table_only = lambda k: k in lev and (k > 2 or gather2)
    # ... and the first layer's partial sums left by the table walk (first_pool: what that launch still owes)
    pool_tables = POOL_TABLES and pool1 and tab1 is not None and 2 in lev and Nc >= batch.POOL_TABLES_MIN_ROWS
    first_pool = None
    pool_parts = {}
    # src[l]: how layer l's launches read tbl[l] where X_l's count rows exist as that table only -- the column ids with the count
    # slots' sources remapped to its rows, and the count launch's OWN rows: from their degrees by these coefficients (l = 1), or
    # through these ids (above that)
    src = {}
    # post_mp.0 can form its operand itself (POOL_POST_FUSED) -- given the partial sums of every layer, see below
    post_fusable = (nb and fuse_post0 and POOL_POST_FUSED and const_input and GEMM_BF16X6 and "post_nk" in pk and L <= 8
                    and batch.max_count_rows() <= 33)
    # the anchor MLP on the classes of anchor operands (acls: the index), the canonical rows as tables per level (ctabs), the
    # pooled sums and all behind them on the pooling classes (pidx: there the first layer's sums, too, come from the tables)
    acls = ctabs = pidx = None
    if (ANCHOR_CLASS_TABLE and DEEP_LAYER_TABLES and L in lev and post_fusable and ANCHOR_POST_FUSED and canon_once
            and L in (2, 5, 8)):
        acls = batch.anchor_class_index(L)
        if CANON_CLASS_TABLES and acls is not None:
            ctabs = batch.canonical_class_tables(L)
        if POOL_CLASS_TABLE and acls is not None and pool_tables and batch.max_count_rows() <= ops.class_rows_pool_max_rows():
            pidx = batch.pool_class_launch_index(L)
    if fpool:
        pbits, pslot, nslots = batch.pool_index()
        if pidx is not None:
            nslots = pidx.nslots                       # (the partial arrays hold the representatives' slots only)
    if const_input:
        x0 = {t: pk["pre"][t][1] for t, *_ in groups}
        src_of_slot = (lambda t, s: ("count" if s < 2 else "canonical")) if nb else (lambda t, s: t)
        xn = torch.empty((N, H), device=dev)
        if pool1:
            pool_parts[1] = torch.empty((nslots, H), device=dev)
        if tab1 is not None:
            coef_c = _first_layer_coef(pk, "count", 4, S, x0, src_of_slot, dev)
            tbl[1] = torch.empty((tab1[0].numel() // S, H), device=dev)
            ops.degree_affine(tab1[0], 0, tbl[1].shape[0], S, coef_c, ops.ACT_RELU, 0.0, tbl[1])
            src[1] = (tab1[2], coef_c, None)
            xn = None
        for t, r0, r1, su in groups:
            if r1 <= r0:
                continue
            coef = _first_layer_coef(pk, t, su, S, x0, src_of_slot, dev)
            if pool1 and t == "count" and pool_tables:
                first_pool = (tbl[1], tab1[1], pool_parts[1])
            elif pool1 and t == "count":
                ops.degree_affine_pool(batch.vrowptr, r1, S, coef, ops.ACT_RELU, 0.0, xn, (pbits, pslot, pool_parts[1]))
            elif t == "canonical" and canon_once:
                pass                                   # (written below, straight into the anchor operand's block 1)
            else:
                ops.degree_affine(batch.vrowptr, r0, r1 - r0, S, coef, ops.ACT_RELU, 0.0, xn)
        X = [None, xn]
    else:
        feat = batch.node_feature
        if feat is None:
            feat = torch.zeros((N, core.input_dim), device=dev)
        x = torch.empty((N, H), device=dev)
        for t, r0, r1, _ in groups:
            wt, b = pk["pre"][t]
            ops.linear_smallk(feat[r0:r1], wt, b, out=x[r0:r1])               # :231
        X = [x]
    first = len(X) - 1
    # emb["canonical"] [B, P] (operand of the anchor MLP): the canonical launches write their column block directly
    # (out2), so no concatenation pass is needed
    canon = torch.empty((B, P), device=dev) if (nb and ctabs is None) else None
    # per-row bound of the anchor operand, left by the launches that write its column blocks (saves the f16x3 GEMM's
    # pre-pass over the operand): only when every block comes from such a launch (constant input, fp16 layer form)
    canon_max = torch.empty((B,), device=dev) if (nb and const_input and f16 and ctabs is None) else None
    if ctabs is not None:
        # ct[l], l = 1 .. L: the distinct canonical rows of X_l, row slices of one buffer; cm[l]: their largest magnitudes
        # (the launches accumulate into zeros what the anchor operand's launches accumulate into the first layer's)
        cbuf, cmax = torch.empty((sum(ctabs.size), H), device=dev), torch.zeros((sum(ctabs.size),), device=dev)
        ct = [None] + [cbuf[o:o + n_] for o, n_ in zip(ctabs.offset, ctabs.size)]
        cm = [None] + [cmax[o:o + n_] for o, n_ in zip(ctabs.offset, ctabs.size)]
        t, r0, r1, su = groups[1]
        ops.degree_affine(ctabs.uptr1, 0, ctabs.size[0], S, _first_layer_coef(pk, t, su, S, x0, src_of_slot, dev),
                          ops.ACT_RELU, 0.0, ct[1], row_absmax=cm[1])
    elif nb and const_input:
        # the closed-form first layer once more for the canonical rows, straight into its column block of the anchor
        # operand (a 1/9-size launch of our own instead of a strided torch copy per pass); it WRITES the row bound the
        # canonical launches below accumulate into, so it runs before them
        t, r0, r1, su = groups[1]
        ops.degree_affine(batch.vrowptr, r0, r1 - r0, S, _first_layer_coef(pk, t, su, S, x0, src_of_slot, dev),
                          ops.ACT_RELU, 0.0, canon[:, H:2 * H], out_row0=0, row_absmax=canon_max)
    for l in range(first, L):                                              # :262-264, :273, :389-395
        last = l == L - 1
        # the last layer's count rows feed nothing but the pooling: with fused pooling they are
        # never stored (the canonical rows still are, they sit at the end of the same tensor)
        xn = None if table_only(l + 1) else torch.empty((N, H), device=dev)
        # layer input, column ids and (count rows) own rows of this layer's launches: X_l itself, or the table of its distinct
        # count rows (src); the table slots' sources stay global ids
        x_src, (vcol_l, coef_l, cls_l) = (tbl[l], src[l]) if l in src else (X[-1], (batch.vcol, None, None))
        for t, r0, r1, su in groups:
            if r1 <= r0:
                continue
            e = pk["layers"][l][t]
            if "wt_tab" in e:
                # canonical rows of X_l
                crows = None if ctabs is not None else canon[:, l * H:(l + 1) * H] if canon_once else X[-1][Nc:]
                tem = temp if isinstance(e.get("wt_mfma_x6"), ops.F16Planes) else 0
                y_row0, vcol_c = Nc, vcol_l
                if tem and l == 1 and ctab is not None:
                    # (the canonical rows of X_1 are a function of their degree tuple: U_c table rows, ids remapped)
                    ytab = _layer2_table(ctab[0], S, _first_layer_coef(pk, "canonical", 2, S, x0, src_of_slot, dev),
                                         e["wt_tab_l64"][tblock:tblock + 1])
                    # (ctab[2] is tab1[2] with the TABLE slots' sources remapped as well; the canonical launch of this layer
                    #  reads slots 0 and 1 only and keeps tab1[2])
                    vcol_c, y_row0 = ctab[2], 0
                elif tem and (l + 1) in lev:
                    # (the representatives' table sources are canonical CLASSES of X_l: the product on their lowest rows)
                    ytab = ops.linear64(ct[l] if ctabs is not None else crows.index_select(0, lev[l + 1].crep),
                                        e["wt_tab_l64"][tblock:tblock + 1])
                    y_row0 = 0
                elif tem:
                    ytab = ops.linear64(crows, e["wt_tab_l64"][tblock:tblock + 1])   # canonical rows x W2 or W3: [B, 64]
                else:
                    ytab = (ops.linear64(crows, e["wt_tab_l64"]) if GEMM_BF16X6 else
                            ops.gemm(crows, e["wt_tab"]))                 # canonical rows x [W2|W3]
                pool = None
                if fpool and "wt_mfma_x6" in e:
                    pool_parts[l + 1] = torch.empty((nslots, H), device=dev)
                    pool = (pbits, pslot, pool_parts[l + 1])
                if (l + 1) in lev:
                    # table level k: the launch on the U_k representatives' compact CSR, sources and own rows in the table before
                    # (own rows from their degrees at k = 2; its pooled partials -- one segment -- are not used), which leaves
                    # table k; then, behind the deepest level's launch, the walk(s) for the partial sums of every table layer --
                    # and the rows of X_2 where the second layer is the only level and they are kept
                    k, lv = l + 1, lev[l + 1]
                    assert tem and pool is not None, "a table level without the narrow fp16 count launch or the fused pooling"
                    tbl[k] = torch.empty(((lv.rep_uptr.numel() - 1) // S, H), device=dev)
                    ops.shmp_layer(x_src, lv.rep_uptr, lv.rep_vcol, 0, tbl[k].shape[0], S, 2, e["wt_mfma_x6"], e["b"], tbl[k],
                                   ytab=ytab, ytab_row0=y_row0, pool=batch.rep_pool_index(k), self_coef=coef_l,
                                   table_empty=tem, self_index=lv.rep_self)
                    if table_only(k):
                        src[k] = (lv.vcol, None, lv.cls)
                    if (k + 1) in lev:
                        continue
                    if pidx is not None:
                        # no walk: every layer's pooled sums on the representatives of the pooling classes, their rows read
                        # through the ids at their original positions
                        assert k == L and first_pool is not None, "pooling classes without the table form of every layer"
                        walk, first_pool = [first_pool] + [(tbl[j], lev[j].cls, pool_parts[j]) for j in range(2, k + 1)], None
                        ops.class_rows_pool(walk, batch.count_ptr, r1 - r0, pidx.prep, pidx.rep_ptr, pidx.bits, pidx.slot,
                                            pidx.nslots)
                        continue
                    for j in range(2, k):
                        pool = pool + (tbl[j], lev[j].cls, pool_parts[j])
                    if first_pool is not None:
                        pool, first_pool = pool + first_pool, None
                    ops.table_rows_pool(tbl[k], lv.cls, r1 - r0, None if (last or table_only(k)) else xn, pool)
                    continue
                ops.shmp_layer(x_src, batch.vrowptr, vcol_c, r0, r1 - r0, S, 2,
                               e.get("wt_mfma_x6", e["wt_mfma"]) if SHMP_BF16X6 else e["wt_mfma"],
                               e["b"], None if (pool is not None and last) else xn, ytab=ytab,
                               ytab_row0=y_row0, pool=pool, self_coef=coef_l, table_empty=tem, self_index=cls_l)
            elif ctabs is not None and t == "canonical":
                # the distinct canonical rows of X_{l+1}: the launch on the representatives' compact CSR, sources in table l of
                # the count rows, own rows gathered from table l of the canonical rows
                rep_uptr, rep_vcol, below = ctabs.levels[l - 1]
                ops.shmp_layer(x_src, rep_uptr, rep_vcol, 0, ctabs.size[l], S, su, e["wt_x6"], e["b"], None, out2=ct[l + 1],
                               row_absmax=cm[l + 1], xself=ct[l].index_select(0, below))
            else:
                canonical, w16 = t == "canonical", isinstance(e.get("wt_x6"), ops.F16Planes)
                once = canon_once and canonical and w16
                ops.shmp_layer(x_src, batch.vrowptr, vcol_l, r0, r1 - r0, S, su,
                               e.get("wt_x6", e["wt"]) if SHMP_BF16X6 else e["wt"], e["b"], None if once else xn,
                               out2=canon[:, (l + 1) * H:(l + 2) * H] if canonical else None,
                               row_absmax=canon_max if (canonical and w16) else None,
                               xself=canon[:, l * H:(l + 1) * H] if once else None)
        X.append(xn)
        assert first_pool is None or (l + 2) in lev, "the first layer's partial sums were left to a launch that was not issued"
        if l in pool_parts:
            # layer l's rows have been consumed (their pooled sums sit in pool_parts[l], their canonical
            # rows in `canon`): release them -- a block then holds three [N, 64] tensors instead of nine,
            # which is what lets InferencePipeline run blocks of tens of millions of rows
            X[l] = _RELEASED
    if nb:
        folded_x0 = GEMM_BF16X6 and const_input    # (_anchor_const_input: K = 512)
        if not folded_x0:
            canon[:, :H] = x0["canonical"].expand(B, H) if const_input else X[0][Nc:]
        seg_ptr = batch.count_ptr
        pool_post = post_fusable and sorted(pool_parts) == list(range(1, L + 1))
        assert pool_post or acls is None, "anchor classes without the partial sums of every layer"
        if pool_post and ANCHOR_POST_FUSED and (canon_max is not None or ctabs is not None) and L in (2, 5, 8):
            _anchor_const_input_weights(pk, gnn)
            aw16, ab16 = pk["anchor_nk_const"]
            w0, b0 = pk["post_nk"][0]
            if acls is not None:
                # the anchor MLP on one representative per class of anchor operands, post_mp.0 reading its rows through the
                # classes: row-local arithmetic on bit-equal operands and row bounds, the pooled sums per neighborhood as before
                if ctabs is not None:
                    a_u = cbuf.index_select(0, ctabs.anchor_rows).view(-1, L * H)
                    bound_u = cmax.index_select(0, ctabs.anchor_rows).view(-1, L).amax(dim=1)
                else:
                    a_u, bound_u = canon[:, H:].index_select(0, acls[1]), canon_max.index_select(0, acls[1])
                anch_tab = ops.gemm_f16x3(a_u, aw16, ab16, act=ops.ACT_LEAKY, slope=0.1, row_scale=bound_u)
                if pidx is not None:
                    # one row per pooling class: the representatives' segments, each layer's combined sum in the segment's
                    # first slot and zeros behind it -- the expressions of the launch below on bit-equal terms
                    return _PostMp0(ops.pool_post(anch_tab, [pool_parts[l] for l in range(1, L + 1)], pidx.bits, pidx.slot,
                                                  pidx.rep_ptr, x0[groups[0][0]], w0, b0, ops.ACT_LEAKY, 0.1,
                                                  anch_row=pidx.anch_row), pidx.pcls)
                return _PostMp0(ops.pool_post(anch_tab, [pool_parts[l] for l in range(1, L + 1)], pbits, pslot, seg_ptr,
                                              x0[groups[0][0]], w0, b0, ops.ACT_LEAKY, 0.1, anch_row=acls[0]))
            return _PostMp0(ops.anchor_pool_post(canon[:, H:], aw16, ab16, canon_max,
                                                 [pool_parts[l] for l in range(1, L + 1)], pbits, pslot,
                                                 seg_ptr, x0[groups[0][0]], w0, b0, ops.ACT_LEAKY, 0.1))
        if folded_x0:
            anch = _anchor_const_input(pk, gnn, canon, row_bound=canon_max)
        elif GEMM_BF16X6:
            anch = _gemm_planes(canon, *pk["anchor_nk"], act=ops.ACT_LEAKY, slope=0.1)
        else:
            aw, ab = pk["anchor"]
            anch = ops.gemm(canon, aw, ab, act=ops.ACT_LEAKY, slope=0.1)   # :69-73
        if pool_post:
            w0, b0 = pk["post_nk"][0]
            return _PostMp0(ops.pool_post(anch, [pool_parts[l] for l in range(1, L + 1)], pbits, pslot, seg_ptr,
                                          x0[groups[0][0]], w0, b0, ops.ACT_LEAKY, 0.1))
    else:
        anch = None                                  # query graphs: no canonical node, no anchor
        seg_ptr = batch.graph_ptr
    pooled = torch.empty((B, P), device=dev)
    if pool_parts:
        # the layers' partial sums, reduced together: one launch for (up to eight of) them instead of one per layer
        ls = sorted(pool_parts)
        ops.pool_reduce_multi([pool_parts[l] for l in ls], pbits, pslot, seg_ptr, B,
                              [None if anch is None else anch[:, l * H:(l + 1) * H] for l in ls],
                              [pooled[:, l * H:(l + 1) * H] for l in ls])
    for l, xl in enumerate(X):                                             # :88-89, :107
        if l in pool_parts:
            continue
        extra = None if anch is None else anch[:, l * H:(l + 1) * H]
        out_l = pooled[:, l * H:(l + 1) * H]
        if xl is None:       # constant X_0: the segment sum is (rows in segment) * x0
            t0 = groups[0][0]
            ck = ("pool0_coef", t0)
            if ck not in pk:
                pk[ck] = torch.stack([x0[t0], torch.zeros(H, device=dev)]).contiguous()
            ops.degree_affine(seg_ptr, 0, B, 1, pk[ck], ops.ACT_NONE, 0.0, out_l, extra=extra)
        else:
            ops.segment_sum(xl[:Nc], seg_ptr, B, extra=extra, out=out_l)
    return pooled


def pack_shmp_stacked(gnn: BaseGNN) -> dict:
    """The folding of pack_shmp -- (U_n W_s)^T per slot, U_x^T, U_n sum_s b_s + c -- for the fused
    training trunk, differentiable and STACKED over the layers: per node type (Wt [L, (S_t+1) 64, 64],
    bias [L, 64]) from a dozen batched torch ops.  (pack_shmp's per-(layer, type) entries cost ~100 small
    differentiable select / cat / add ops per step, and their backward as many zero-fills, copies and full-size
    accumulations: half of the replayed step's GPU time in round 2.)"""
    core = gnn.gnn_core
    L = core.layer_num
    out = {}
    for t in core.row_types():
        keys = core.slot_keys(t)
        uniq = list(dict.fromkeys(keys))                 # one bias per edge TYPE (use_tconv=False ties two slots)
        U = torch.stack([core.update(l, t).weight for l in range(L)])                    # [L, 64, 128]
        c = torch.stack([core.update(l, t).bias for l in range(L)])                      # [L, 64]
        Un, Ux = U[:, :, :H], U[:, :, H:]
        W = torch.stack([core.conv(l, k).lin.weight for l in range(L) for k in keys]).view(L, len(keys), H, H)
        bs = torch.stack([core.conv(l, k).lin.bias for l in range(L) for k in uniq]).view(L, len(uniq), H).sum(1)
        folded = torch.matmul(Un.unsqueeze(1), W).transpose(-1, -2)                       # (U_n W_s)^T
        Wt = torch.cat([folded, Ux.transpose(-1, -2).unsqueeze(1)], dim=1).reshape(L, (len(keys) + 1) * H, H)
        fb = _mv(Un, bs) + c
        out[t] = (Wt, fb)
    return out


def fold_shmp_native(gnn: BaseGNN, t: str):
    """(Wt [L, (S_t+1) 64, 64], fb [L, 64]) of row type ``t`` -- pack_shmp_stacked's folding -- by desco_fold_shmp_fwd
    from the raw parameters, differentiable through autograd.FoldShmp (gradients in one flat buffer, no torch op)."""
    from . import autograd as AG
    specs = gnn.__dict__.setdefault("_fold_specs", {})
    sp = specs.get(t)
    if sp is None or not sp.valid():
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("fold_shmp_native: the parameter address table has to be (re)built, which uploads it -- "
                               "not inside a hipGraph capture; run one eager step after replacing parameters")
        sp = specs[t] = AG.FoldSpec(gnn.gnn_core, t)
    return AG.FoldShmp.apply(sp, *sp.params)


POST_DROP_SITE = 200      # dropout site of post_mp.1 (the layers use 2 l + row type)


def shmp_forward_train(gnn: BaseGNN, batch, drop_key: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable twin of ``shmp_forward`` (same math; every forward and backward op is a C-ABI kernel launch of
    desco_amd.autograd).  ``drop_key``: the (seed, step) key of this pass's dropout (ops.rng_next), drawn here when
    None -- callers that run two models on two streams draw both keys first, on one stream
    (NeighborhoodCountingModel.train_forward)."""
    from . import autograd as AG
    core = gnn.gnn_core
    dev = batch.vrowptr.device
    N, S = batch.num_rows, batch.slots
    # --neigh_dropout > 0 (default 0.0, config.py:251): F.dropout after every layer's relu (gnn_model.py:274) and the
    # nn.Dropout of post_mp.1 (:46), in training mode: counter-based factors inside the fused nodes' epilogues
    # (autograd.ShmpTrunk / ShmpTrunkSmall / Mlp), as in the gossip model
    p_layer = float(core.dropout or 0.0) if gnn.training else 0.0
    p_post = float(gnn.post_mp[1].p or 0.0) if gnn.training else 0.0
    drop = p_layer > 0.0 or p_post > 0.0
    has_anchor = isinstance(batch, NeighborhoodBatch)
    if has_anchor:
        Nc = batch.num_count
        groups = [("count", 0, Nc, 4), ("canonical", Nc, N, 2)]
    else:
        groups = [("union_node", 0, N, 2)]
    feat = batch.node_feature
    if feat is None:
        feat = batch.__dict__.get("_zero_feat")          # ZeroNodeFeat: a constant of the batch, made once
        if feat is None or feat.shape[1] != core.input_dim:
            feat = batch.__dict__["_zero_feat"] = torch.zeros((N, core.input_dim), device=dev)
    # the query graphs (<= 144 rows): the whole trunk in one launch per direction (autograd.ShmpTrunkSmall; only its
    # per-graph kernels carry the dropout factors)
    small = not has_anchor and S == 2 and core.layer_num >= 1 and 0 < N <= ops.shmp_trunk_small_max_rows()
    if small and drop and not AG.ShmpTrunkSmall.per_graph(batch):
        small = False
    if drop and drop_key is None:
        drop_key = ops.rng_next(dev)
    ldrop = (drop_key, p_layer) if p_layer > 0.0 else None
    # The whole layer loop + anchor + pooling as one autograd node (autograd.ShmpTrunk) on weights folded in
    # stacked form.  Everything between the parameters and that node is this library's kernels too (round 5): the
    # folding reads the parameters through an address table (autograd.FoldShmp), the K-major copies of pre_mp /
    # anchor_mlp / post_mp are one copy2d launch (autograd.TransposedMany), pre_mp writes one buffer (PreLinear).
    lins = [core.pre_lin(t) for t, *_ in groups] + ([gnn.anchor_mlp[0]] if has_anchor else []) + \
           [gnn.post_mp[i] for i in (0, 3, 5, 7)]
    wts = AG.TransposedMany.apply(*[m.weight for m in lins])
    ng = len(groups)
    pre = []
    for g in range(ng):
        pre += [wts[g], lins[g].bias]
    x = AG.PreLinear.apply(feat, groups, *pre)
    flat = [wts[ng], gnn.anchor_mlp[0].bias] if has_anchor else []
    for t, *_ in groups:
        flat += list(fold_shmp_native(gnn, t))
    if small:
        pooled = AG.ShmpTrunkSmall.apply(x, batch, ldrop, *flat)
    else:
        pooled = AG.ShmpTrunk.apply(x, batch, groups, has_anchor, ldrop, *flat)
    pw = wts[ng + (1 if has_anchor else 0):]
    post = [v for j, i in enumerate((0, 3, 5, 7)) for v in (pw[j], gnn.post_mp[i].bias)]
    pdrop = ops.DropSite(drop_key, POST_DROP_SITE, p_post) if p_post > 0.0 else None
    # post_mp: the four Linears and their backward as one autograd node (activation derivatives in the GEMM epilogues,
    # one launch pair for all weight gradients)
    return AG.Mlp.apply(pooled, ((ops.ACT_LEAKY, 0.1), (ops.ACT_RELU, 0.0), (ops.ACT_RELU, 0.0), (ops.ACT_NONE, 0.0)),
                        tuple(gnn.post_mp[i].weight for i in (0, 3, 5, 7)), pdrop, *post)


# -------------------------------------------------------------------------------------------------
# neighborhood / query models of other widths than 64 (the wide path)
# -------------------------------------------------------------------------------------------------
# the wide layers as one fused launch per node-type group and layer (desco_shmp_layer_wide_f16x3_f32); False: the
# gather (desco_csr_gather_sum_wide_f32) + f16x3 GEMM form, for A/B runs and as the fused kernel's cross-check
SHMP_WIDE_FUSED = os.environ.get("DESCO_SHMP_WIDE_FUSED", "1") != "0"


def _pad_blocks(w: torch.Tensor, h: int, wp: int, nrow: int, ncol: int) -> torch.Tensor:
    """[nrow h, ncol h] -> [nrow wp, ncol wp]: every h x h block zero-padded on its own (differentiable)"""
    w4 = w.reshape(nrow, h, ncol, h)
    return torch.nn.functional.pad(w4, (0, wp - h, 0, 0, 0, wp - h)).reshape(nrow * wp, ncol * wp)


def _pad_to(w: torch.Tensor, *shape) -> torch.Tensor:
    """zero-pad w at the end of every dimension to ``shape`` (differentiable)"""
    pads = []
    for d in reversed(range(w.dim())):
        pads += [0, shape[d] - w.shape[d]]
    return torch.nn.functional.pad(w, pads)


def pack_shmp_wide(gnn: BaseGNN, planes: bool = True) -> dict:
    """The operands of pack_shmp for a model of width h != 64, zero-padded to wp = padded_width(h) block by block
    (pre_mp rows, every slot block and the self block of a folded layer weight, every layer block of the anchor and of
    post_mp.0), so that the padded channels are exactly 0 after every activation.  K-major ([in, out]) matrices;
    ``planes``: also the fp16 planes of the f16x3 kernels (inference).  Differentiable (training)."""
    core = gnn.gnn_core
    h = core.hidden_dim
    wp = padded_width(h)
    L = core.layer_num
    pk = {"h": h, "wp": wp, "pre": {}, "layers": []}
    for t in core.row_types():
        lin = core.pre_lin(t)
        pk["pre"][t] = (_pad_to(lin.weight.t(), lin.in_features, wp).contiguous(), _pad_to(lin.bias, wp).contiguous())
    for l in range(L):
        per_type = {}
        for t in core.row_types():
            U, c = core.update(l, t).weight, core.update(l, t).bias
            Un, Ux = U[:, :h], U[:, h:]
            keys = core.slot_keys(t)
            blocks = [(Un @ core.conv(l, k).lin.weight).t() for k in keys]                  # (U_n W_s)^T
            blocks.append(Ux.t())
            bsum = sum(core.conv(l, k).lin.bias for k in dict.fromkeys(keys))                 # one bias per edge TYPE
            wt = _pad_blocks(torch.cat(blocks, 0), h, wp, len(blocks), 1).contiguous()      # [(S+1) wp, wp]
            e = {"wt": wt, "b": _pad_to(_mv(Un, bsum) + c, wp).contiguous(), "slots": len(keys)}
            if planes:
                e["w16"] = ops.split_f16_planes(wt.t())
            per_type[t] = e
        pk["layers"].append(per_type)
    return _pack_wide_tail(gnn, pk, planes)


def _pack_wide_tail(gnn: BaseGNN, pk: dict, planes: bool) -> dict:
    """the anchor MLP and post_mp operands of the padded-operand paths (pack_shmp_wide, pack_plain), padded block by block"""
    core = gnn.gnn_core
    h, wp, L = pk["h"], pk["wp"], core.layer_num
    if core.row_types() != QUERY_NODE_TYPES:
        aw = gnn.anchor_mlp[0]
        pk["anchor"] = (_pad_blocks(aw.weight.t(), h, wp, L + 1, L + 1).contiguous(),
                        torch.nn.functional.pad(aw.bias.view(L + 1, h), (0, wp - h)).reshape(-1).contiguous())
        if planes:
            pk["anchor16"] = ops.split_f16_planes(pk["anchor"][0].t())
    p0 = gnn.post_mp[0]
    n0 = padded_width(p0.out_features)
    pk["post"] = [(_pad_to(torch.nn.functional.pad(p0.weight.t().reshape(L + 1, h, -1), (0, 0, 0, wp - h)).reshape(
        (L + 1) * wp, -1), (L + 1) * wp, n0).contiguous(), _pad_to(p0.bias, n0).contiguous())]
    for i in (3, 5, 7):
        m = gnn.post_mp[i]
        pk["post"].append((_pad_to(m.weight.t(), padded_width(m.in_features), padded_width(m.out_features)).contiguous(),
                           _pad_to(m.bias, padded_width(m.out_features)).contiguous()))
    return pk


def _wide_groups(batch):
    if isinstance(batch, NeighborhoodBatch):
        Nc = batch.num_count
        return Nc, [("count", 0, Nc, 4), ("canonical", Nc, batch.num_rows, 2)], batch.count_ptr
    return batch.num_rows, [("union_node", 0, batch.num_rows, 2)], batch.graph_ptr


def _wide_zero_feat(gnn: BaseGNN, batch, N: int, dev):
    """ZeroNodeFeat: the all-zero input rows, made once per batch by this library's fill"""
    feat = batch.__dict__.get("_zero_feat")
    if feat is None or feat.shape[1] != gnn.gnn_core.input_dim:
        feat = batch.__dict__["_zero_feat"] = ops.zeros((N, gnn.gnn_core.input_dim), dev)
    return feat


def shmp_forward_wide(gnn: BaseGNN, batch) -> torch.Tensor:
    """Inference of a model of width h != 64 (BaseGNN.forward, gnn_model.py:58-109) on the zero-padded operands of
    pack_shmp_wide -> graph embeddings [B, padded_width(output_dim)]: pre_mp (linear_smallk), per layer and node-type
    group one desco_shmp_layer_wide_f16x3_f32 launch (the canonical launches also write their column block of the
    anchor operand), the anchor on the f16x3 GEMM, pooling by segment_sum with the anchor block as `extra`, post_mp on
    the fp32 GEMM."""
    pk = gnn.packed()
    core = gnn.gnn_core
    wp = pk["wp"]
    dev = batch.vrowptr.device
    N, S, B, L = batch.num_rows, batch.slots, batch.num_graphs, core.layer_num
    Nc, groups, seg_ptr = _wide_groups(batch)
    nb = isinstance(batch, NeighborhoodBatch)
    feat = batch.node_feature
    if feat is None:
        feat = _wide_zero_feat(gnn, batch, N, dev)
    x = torch.empty((N, wp), device=dev)
    for t, r0, r1, _ in groups:
        if r1 > r0:
            ops.linear_smallk(feat[r0:r1], *pk["pre"][t], out=x[r0:r1])                # :231
    canon = torch.empty((B, (L + 1) * wp), device=dev) if nb else None             # emb["canonical"]
    if nb and N > Nc:
        ops.copy2d_multi([(x[Nc:], canon[:, :wp])])
    X = [x]
    for l in range(L):
        xn = torch.empty((N, wp), device=dev)
        cblock = canon[:, (l + 1) * wp:(l + 2) * wp] if nb else None
        if SHMP_WIDE_FUSED:
            for t, r0, r1, su in groups:                                               # :262-264, :273
                if r1 > r0:
                    e = pk["layers"][l][t]
                    ops.shmp_layer_wide(X[-1], batch.vrowptr, batch.vcol, S, r0, r1 - r0, su, e["w16"], e["b"], out=xn,
                                        out2=cblock if t == "canonical" else None)
        else:
            agg = ops.csr_gather_sum_wide(X[-1], batch.vrowptr, batch.vcol, N, S)     # [N, S wp]
            for t, r0, r1, su in groups:
                if r1 > r0:
                    e = pk["layers"][l][t]
                    ops.gemm_f16x3(agg[r0:r1, :su * wp], e["w16"], e["b"], a2=X[-1][r0:r1], act=ops.ACT_RELU,
                                   out=xn[r0:r1])
            if nb and N > Nc:
                ops.copy2d_multi([(xn[Nc:], cblock)])
        X.append(xn)
    pooled = torch.empty((B, (L + 1) * wp), device=dev)
    anch = ops.gemm_f16x3(canon, pk["anchor16"], pk["anchor"][1], act=ops.ACT_LEAKY, slope=0.1) if nb else None
    for l, xl in enumerate(X):                                                         # :88-89, :107
        ops.segment_sum(xl[:Nc], seg_ptr, B, extra=None if anch is None else anch[:, l * wp:(l + 1) * wp],
                        out=pooled[:, l * wp:(l + 1) * wp])
    (w0, b0), (w3, b3), (w5, b5), (w7, b7) = pk["post"]                                # :44-53
    h = ops.gemm(pooled, w0, b0, act=ops.ACT_LEAKY, slope=0.1)
    h = ops.gemm(h, w3, b3, act=ops.ACT_RELU)
    h = ops.gemm(h, w5, b5, act=ops.ACT_RELU)
    return ops.gemm(h, w7, b7)


# dropout sites of the wide training pass: layer l's rows 2 l, post_mp.1 POST_DROP_SITE
def wide_layer_drop_site(l: int) -> int:
    return 2 * l


def shmp_forward_train_wide(gnn: BaseGNN, batch, drop_key: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable twin of ``shmp_forward_wide`` -> [B, padded_width(output_dim)]: the per-op autograd composition
    (SmallKLinear, GatherSumWide, Linear, SegmentSumWide, Linear) on the operands pack_shmp_wide pads with differentiable
    torch ops, so that the gradients reach the true-width parameters (the padded channels get none).  --neigh_dropout:
    the counter-based factors of ops.dropout_mask (sites wide_layer_drop_site(l) and POST_DROP_SITE of ``drop_key``)."""
    from . import autograd as AG
    import torch.nn.functional as F
    core = gnn.gnn_core
    dev = batch.vrowptr.device
    N, S, L = batch.num_rows, batch.slots, core.layer_num
    Nc, groups, seg_ptr = _wide_groups(batch)
    nb = isinstance(batch, NeighborhoodBatch)
    p_layer = float(core.dropout or 0.0) if gnn.training else 0.0
    p_post = float(gnn.post_mp[1].p or 0.0) if gnn.training else 0.0
    if (p_layer > 0.0 or p_post > 0.0) and drop_key is None:
        drop_key = ops.rng_next(dev)
    pk = pack_shmp_wide(gnn, planes=False)
    wp = pk["wp"]
    feat = batch.node_feature
    if feat is None:
        feat = _wide_zero_feat(gnn, batch, N, dev)
    ti = batch.train_index()
    x = torch.cat([AG.SmallKLinear.apply(feat[r0:r1], *pk["pre"][t]) for t, r0, r1, _ in groups], 0)
    X = [x]
    for l in range(L):
        agg = AG.GatherSumWide.apply(X[-1], batch.vrowptr, batch.vcol, ti["t_rowptr"], ti["t_col"], N, S)
        parts = []
        for t, r0, r1, su in groups:
            e = pk["layers"][l][t]
            parts.append(AG.Linear.apply(agg[r0:r1, :su * wp], X[-1][r0:r1], e["wt"], e["b"], ops.ACT_RELU, 0.0))
        xl = torch.cat(parts, 0)
        if p_layer > 0.0:                                                              # gnn_model.py:274
            xl = xl * ops.dropout_mask(ops.DropSite(drop_key, wide_layer_drop_site(l), p_layer), N, wp)
        X.append(xl)
    if nb:
        canon = torch.cat([xl[Nc:] for xl in X], dim=1)
        aw, ab = pk["anchor"]
        anch = AG.Linear.apply(canon, None, aw, ab, ops.ACT_LEAKY, 0.1)
        pooled = torch.cat([AG.SegmentSumWide.apply(xl[:Nc], seg_ptr, ti["seg_id"], ti["ident_ptr"],
                                                    anch[:, l * wp:(l + 1) * wp].contiguous())
                            for l, xl in enumerate(X)], dim=1)
    else:
        pooled = torch.cat([AG.SegmentSumWide.apply(xl, seg_ptr, ti["seg_id"], ti["ident_ptr"], None) for xl in X], dim=1)
    (w0, b0), (w3, b3), (w5, b5), (w7, b7) = pk["post"]
    h = AG.Linear.apply(pooled, None, w0, b0, ops.ACT_NONE, 0.0)
    if p_post > 0.0:                                                                   # post_mp.1 (gnn_model.py:46)
        h = h * ops.dropout_mask(ops.DropSite(drop_key, POST_DROP_SITE, p_post), h.shape[0], h.shape[1])
    h = F.leaky_relu(h, 0.1)
    h = AG.Linear.apply(h, None, w3, b3, ops.ACT_RELU, 0.0)
    h = AG.Linear.apply(h, None, w5, b5, ops.ACT_RELU, 0.0)
    return AG.Linear.apply(h, None, w7, b7, ops.ACT_NONE, 0.0)


# -------------------------------------------------------------------------------------------------
# plain GIN / GCN neighborhood / query models (--neigh_conv_type GIN / GCN, homogeneous)
# -------------------------------------------------------------------------------------------------
# a plain layer as ONE fused launch (desco_plain_layer_f16x3_f32: gather, the eps x term, one or two products, relu);
# False: the un-fused composition (desco_csr_gather_sum_wide_f32 with slots = 1, the eps x term, gemm_f16x3 once or
# twice), for A/B runs and as the fused kernel's cross-check
PLAIN_FUSED = os.environ.get("DESCO_PLAIN_FUSED", "1") != "0"


def pack_plain(gnn: BaseGNN, planes: bool = True) -> dict:
    """The operands of a plain GIN / GCN model, zero-padded to wp = padded_width(h) like pack_shmp_wide's (K-major
    [in, out] matrices; ``planes``: also the fp16 planes of the f16x3 kernels).  Per layer ``wt1``, ``b1`` and, for GIN,
    ``wt2``, ``b2``, ``eps`` (the buffer itself, read on the device).  GIN's constant 1 -- the reference's
    ``x_neigh + (1 + eps x)`` -- is folded into the first bias over the TRUE width, b1' = b1 + W1 1, so that the padded
    channels stay exactly 0.  Differentiable (training)."""
    core = gnn.gnn_core
    h = core.hidden_dim
    wp = padded_width(h)
    lin = core.pre_mp[0]
    pre = (_pad_to(lin.weight.t(), lin.in_features, wp).contiguous(), _pad_to(lin.bias, wp).contiguous())
    pk = {"h": h, "wp": wp, "pre": {t: pre for t in core.row_types()}, "layers": []}
    for l in range(core.layer_num):
        if core.conv_type == "GIN":
            u = core.updates[l]
            W1, W2 = u[0].weight, u[2].weight
            e = {"wt1": _pad_to(W1.t(), wp, wp).contiguous(), "b1": _pad_to(u[0].bias + W1.sum(1), wp).contiguous(),
                 "wt2": _pad_to(W2.t(), wp, wp).contiguous(), "b2": _pad_to(u[2].bias, wp).contiguous(),
                 "eps": core.eps[l].eps}
        else:
            c = core.convs[l]
            e = {"wt1": _pad_to(c.lin.weight.t(), wp, wp).contiguous(), "b1": _pad_to(c.bias, wp).contiguous()}
        if planes:
            e["w1_16"] = ops.split_f16_planes(e["wt1"].t())
            if "wt2" in e:
                e["w2_16"] = ops.split_f16_planes(e["wt2"].t())
        pk["layers"].append(e)
    return _pack_wide_tail(gnn, pk, planes)


def _plain_tail(pk, batch, X, canon, Nc, seg_ptr, B):
    """the wide path's tail: anchor on the f16x3 GEMM, pooling with the anchor block as ``extra``, fp32 post_mp"""
    wp = pk["wp"]
    dev = X[0].device
    pooled = torch.empty((B, len(X) * wp), device=dev)
    anch = None if canon is None else ops.gemm_f16x3(canon, pk["anchor16"], pk["anchor"][1], act=ops.ACT_LEAKY, slope=0.1)
    for l, xl in enumerate(X):                                                         # :88-89, :107
        ops.segment_sum(xl[:Nc], seg_ptr, B, extra=None if anch is None else anch[:, l * wp:(l + 1) * wp],
                        out=pooled[:, l * wp:(l + 1) * wp])
    (w0, b0), (w3, b3), (w5, b5), (w7, b7) = pk["post"]                                # :44-53
    h = ops.gemm(pooled, w0, b0, act=ops.ACT_LEAKY, slope=0.1)
    h = ops.gemm(h, w3, b3, act=ops.ACT_RELU)
    h = ops.gemm(h, w5, b5, act=ops.ACT_RELU)
    return ops.gemm(h, w7, b7)


def plain_forward(gnn: BaseGNN, batch) -> torch.Tensor:
    """Inference of a plain GIN / GCN model (BaseGNN.forward with use_hetero False, gnn_model.py:58-109, :262-270) on the
    operands of pack_plain -> graph embeddings [B, padded_width(output_dim)]: one linear_smallk for pre_mp over all
    rows, ONE desco_plain_layer_f16x3_f32 launch per layer over all N rows of the batch's plain CSR (it also writes the
    canonical rows into their column block of the anchor operand), then shmp_forward_wide's tail."""
    pk = gnn.packed()
    core = gnn.gnn_core
    wp = pk["wp"]
    dev = batch.vrowptr.device
    N, B, L = batch.num_rows, batch.num_graphs, core.layer_num
    Nc, groups, seg_ptr = _wide_groups(batch)
    nb = isinstance(batch, NeighborhoodBatch)
    rowptr, col = batch.plain_csr()
    feat = batch.node_feature
    if feat is None:
        feat = _wide_zero_feat(gnn, batch, N, dev)
    x = torch.empty((N, wp), device=dev)
    ops.linear_smallk(feat, *pk["pre"][groups[0][0]], out=x)                           # :231
    canon = torch.empty((B, (L + 1) * wp), device=dev) if nb else None             # emb["canonical"]
    anchored = nb and N > Nc
    if anchored:
        ops.copy2d_multi([(x[Nc:], canon[:, :wp])])
    X = [x]
    for l in range(L):
        e = pk["layers"][l]
        xn = torch.empty((N, wp), device=dev)
        cblock = canon[:, (l + 1) * wp:(l + 2) * wp] if anchored else None
        if PLAIN_FUSED:
            ops.plain_layer(X[-1], rowptr, col, 0, N, e["w1_16"], e["b1"], e.get("w2_16"), e.get("b2"),
                            self_scale=e.get("eps"), out=xn, out2=cblock, out2_row0=Nc)            # :262-273
        else:
            z = ops.csr_gather_sum_wide(X[-1], rowptr, col, N, 1)
            if "eps" in e:
                z = z + e["eps"] * X[-1]
            if "w2_16" in e:
                t = ops.gemm_f16x3(z, e["w1_16"], e["b1"], act=ops.ACT_RELU)
                ops.gemm_f16x3(t, e["w2_16"], e["b2"], act=ops.ACT_RELU, out=xn)
            else:
                ops.gemm_f16x3(z, e["w1_16"], e["b1"], act=ops.ACT_RELU, out=xn)
            if anchored:
                ops.copy2d_multi([(xn[Nc:], cblock)])
        X.append(xn)
    return _plain_tail(pk, batch, X, canon if nb else None, Nc, seg_ptr, B)


def plain_forward_train(gnn: BaseGNN, batch, drop_key: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable twin of ``plain_forward`` -> [B, padded_width(output_dim)]: the per-op autograd composition of
    shmp_forward_train_wide (SmallKLinear, GatherSumWide with slots = 1, Linear, SegmentSumWide) on operands padded with
    differentiable torch ops, so that the gradients reach the true-width parameters only; ``eps`` is a buffer and gets
    none.  The batch CSR is symmetric, so the transposed index of the plain CSR is the plain CSR itself.  Dropout: the
    counter-based factors at sites wide_layer_drop_site(l) and POST_DROP_SITE of ``drop_key``."""
    from . import autograd as AG
    import torch.nn.functional as F
    core = gnn.gnn_core
    dev = batch.vrowptr.device
    N, L = batch.num_rows, core.layer_num
    Nc, groups, seg_ptr = _wide_groups(batch)
    nb = isinstance(batch, NeighborhoodBatch)
    p_layer = float(core.dropout or 0.0) if gnn.training else 0.0
    p_post = float(gnn.post_mp[1].p or 0.0) if gnn.training else 0.0
    if (p_layer > 0.0 or p_post > 0.0) and drop_key is None:
        drop_key = ops.rng_next(dev)
    pk = pack_plain(gnn, planes=False)
    wp = pk["wp"]
    feat = batch.node_feature
    if feat is None:
        feat = _wide_zero_feat(gnn, batch, N, dev)
    ti = batch.train_index()
    rowptr, col = batch.plain_csr()
    X = [AG.SmallKLinear.apply(feat, *pk["pre"][groups[0][0]])]
    for l in range(L):
        e = pk["layers"][l]
        z = AG.GatherSumWide.apply(X[-1], rowptr, col, rowptr, col, N, 1)
        if "eps" in e:
            z = z + e["eps"] * X[-1]
            t = AG.Linear.apply(z, None, e["wt1"], e["b1"], ops.ACT_RELU, 0.0)
            xl = AG.Linear.apply(t, None, e["wt2"], e["b2"], ops.ACT_RELU, 0.0)
        else:
            xl = AG.Linear.apply(z, None, e["wt1"], e["b1"], ops.ACT_RELU, 0.0)
        if p_layer > 0.0:                                                              # gnn_model.py:274
            xl = xl * ops.dropout_mask(ops.DropSite(drop_key, wide_layer_drop_site(l), p_layer), N, wp)
        X.append(xl)
    if nb:
        canon = torch.cat([xl[Nc:] for xl in X], dim=1)
        aw, ab = pk["anchor"]
        anch = AG.Linear.apply(canon, None, aw, ab, ops.ACT_LEAKY, 0.1)
        pooled = torch.cat([AG.SegmentSumWide.apply(xl[:Nc], seg_ptr, ti["seg_id"], ti["ident_ptr"],
                                                    anch[:, l * wp:(l + 1) * wp].contiguous())
                            for l, xl in enumerate(X)], dim=1)
    else:
        pooled = torch.cat([AG.SegmentSumWide.apply(xl, seg_ptr, ti["seg_id"], ti["ident_ptr"], None) for xl in X], dim=1)
    (w0, b0), (w3, b3), (w5, b5), (w7, b7) = pk["post"]
    h = AG.Linear.apply(pooled, None, w0, b0, ops.ACT_NONE, 0.0)
    if p_post > 0.0:                                                                   # post_mp.1 (gnn_model.py:46)
        h = h * ops.dropout_mask(ops.DropSite(drop_key, POST_DROP_SITE, p_post), h.shape[0], h.shape[1])
    h = F.leaky_relu(h, 0.1)
    h = AG.Linear.apply(h, None, w3, b3, ops.ACT_RELU, 0.0)
    h = AG.Linear.apply(h, None, w5, b5, ops.ACT_RELU, 0.0)
    return AG.Linear.apply(h, None, w7, b7, ops.ACT_NONE, 0.0)


# -------------------------------------------------------------------------------------------------
# gossip path
# -------------------------------------------------------------------------------------------------
# test switch: run the dropout form of the training kernels at p = 0 too (must not change a bit: factor 1 everywhere)
DROPOUT_AT_ZERO = False


def gossip_emb_width(core: BaseGNNCore) -> int:
    """width of the query embeddings a gossip model reads (emb_channels = --neigh_hidden_dim, main.py:145).  The layer-0
    input is [E | pre_mp(x)], so E's width decides where the pre_mp and h_l column blocks of lin_com / lin_update of layer
    0 and of post_mp.0 start; H (the module constant) is the gossip model's own width."""
    return int(core.kwargs.get("emb_channels", H))


def pack_gossip(gnn: BaseGNN, bf16_planes: bool = True) -> dict:
    core = gnn.gnn_core
    He = gossip_emb_width(core)
    if core.layer_num < 1 or not core.input_pattern_emb or core.input_dim != 1:
        raise NotImplementedError(
            "gossip kernels implement GossipConv layers with input_dim 1 and the query embedding as input "
            "(config.py:312-322, main.py:316-325)")
    pre = core.pre_mp[0]
    pk = {"w_pre": pre.weight[:, 0].contiguous(), "b_pre": pre.bias.contiguous(),
          "post": [_lin_t(gnn.post_mp[i]) for i in (3, 5)], "w7": gnn.post_mp[7].weight[0].contiguous(),
          "b7": float(gnn.post_mp[7].bias[0]), "qcache": None}
    if core.layer_num != 2:
        return _pack_gossip_deep(gnn, pk)
    c1 = core.convs[1]
    D1 = c1.lin_update.weight
    D1a, D1b = D1[:, :H], D1[:, H:]
    wt1 = torch.cat([(D1a @ c1.lin_com.weight).t(), D1b.t()], 0).contiguous()   # [128,64]
    pk["u1"] = _mv(D1a, c1.lin_com.bias)
    pk["d1"] = c1.lin_update.bias.contiguous()
    P0 = gnn.post_mp[0].weight
    wtp = torch.cat([P0[:, He + H:He + 2 * H].t(), P0[:, He + 2 * H:He + 3 * H].t()], 0).contiguous()
    pk["fused_w1"] = wt1.t().contiguous()                       # [64,128]
    pk["fused_wp"] = wtp.t().contiguous()                       # [64,128]
    pk["fused_w3"] = gnn.post_mp[3].weight.contiguous()         # [64,64]  (already [out, in])
    pk["fused_w5"] = gnn.post_mp[5].weight.contiguous()         # [256,64]
    if bf16_planes:     # bf16 planes (hi, mid, lo) of the n-major matrices: the fused kernel's operands
        for k in ("fused_w1", "fused_wp", "fused_w3", "fused_w5"):
            pk[k + "s"] = ops.split_bf16_planes(pk[k])
        # ... and the fp16 (hi, lo) weight stream of the three-product kernel
        pk["wstream"], pk["winv"] = ops.gossip_f16_stream(*[ops.split_f16_planes(pk[k]) for k in
                                                            ("fused_w1", "fused_wp", "fused_w3", "fused_w5")])
    return pk


def _pack_gossip_deep(gnn: BaseGNN, pk: dict) -> dict:
    """Operands of a depth-L gossip model (L != 2) beyond pack_gossip's head ``pk``: per layer l >= 1 the
    folded weight W_l = [(D_a C)^T; D_b^T]_l as fp16 planes of its n-major form, u_l = D_a c_l and d_l, and the
    post_mp.0 blocks P0_l of h_1 .. h_L (n-major [64, 64] = the block of the torch weight as it is stored)."""
    core = gnn.gnn_core
    He = gossip_emb_width(core)
    L = core.layer_num
    P0 = gnn.post_mp[0].weight
    layers = []
    for l in range(1, L):
        c = core.convs[l]
        Da, Db = c.lin_update.weight[:, :H], c.lin_update.weight[:, H:]
        w_nk = torch.cat([Da @ c.lin_com.weight, Db], 1).contiguous()               # [64 out, 128 in] = W_l^T
        layers.append({"w": ops.split_f16_planes(w_nk), "u": _mv(Da, c.lin_com.bias).contiguous(),
                       "d": c.lin_update.bias.contiguous()})
    pk["deep"] = layers
    pk["deep_p"] = [ops.split_f16_planes(P0[:, He + l * H:He + (l + 1) * H].contiguous()) for l in range(1, L + 1)]
    if L == 1:      # h1 . P0_1 on the fp32 matrix pipe (no gossip layer to carry it)
        pk["p1t"] = P0[:, He + H:He + 2 * H].t().contiguous()
    return pk


def _gossip_layer0_terms(core: BaseGNNCore, post0: nn.Linear, E: torch.Tensor, w_pre: torch.Tensor,
                         b_pre: torch.Tensor):
    """The per-query terms of a gossip pass, from the query embeddings E [Q, He] and pre_mp's weight
    column / bias: the gates g_l [Q] of every layer; p, z [Q, 64] and r, t [64] of the closed-form layer 0
    (h1 = relu(a0 p + b0 r + x t + z) per row, a0 / b0 the gated degree sums); zp [Q, 64] and tp [64] of post_mp.0's
    E and pre_mp blocks (zp + x tp).  Differentiable; the callers stack and expand them into their operand layouts."""
    He = gossip_emb_width(core)
    c0 = core.convs[0]
    C0, D0, P0 = c0.lin_com.weight, c0.lin_update.weight, post0.weight
    g = [c._gate_value(E).reshape(-1) for c in core.convs]                              # gnn_model.py:340
    a_q = E @ C0[:, :He].t() + (_mv(C0[:, He:], b_pre) + c0.lin_com.bias)                # lin_com(h0) const part
    v = _mv(C0[:, He:], w_pre)
    D0a, D0b, D0c = D0[:, :H], D0[:, H:H + He], D0[:, H + He:]
    p = a_q @ D0a.t()
    r = _mv(D0a, v)
    t = _mv(D0c, w_pre)
    z = E @ D0b.t() + (_mv(D0c, b_pre) + c0.lin_update.bias)
    tp = _mv(P0[:, He:He + H], w_pre)
    zp = E @ P0[:, :He].t() + (_mv(P0[:, He:He + H], b_pre) + post0.bias)
    return g, p, r, t, z, tp, zp


def _gossip_query_terms_deep(gnn: BaseGNN, pk: dict, query_emb: torch.Tensor) -> dict:
    """Per-query operands of a depth-L model: gates g_l, V0 = [p, r, t, z] of the closed-form layer 0 against the row
    constants (a0, b0, x, 1), V_l = [u_l, g_l u_l, d_l] against C3 = (deg_hi, deg_lo - deg_hi, 1), and the
    accumulator's start [0, 0, tp, zp] (zp + x tp: the E and pre_mp blocks of post_mp.0)."""
    key = (query_emb.data_ptr(), query_emb._version, tuple(query_emb.shape))
    if pk["qcache"] is not None and pk["qcache"][0] == key:
        return pk["qcache"][1]
    E = query_emb.float()
    Q = E.shape[0]
    g, p, r, t, z, tp, zp = _gossip_layer0_terms(gnn.gnn_core, gnn.post_mp[0], E, pk["w_pre"], pk["b_pre"])
    q = {"g": [gl.contiguous() for gl in g]}
    q["V0"] = torch.stack([p, r.expand(Q, H), t.expand(Q, H), z], 1).contiguous()     # [Q,4,64]
    zero = torch.zeros_like(zp)
    q["Vacc"] = torch.stack([zero, zero, tp.expand(Q, H), zp], 1).contiguous()
    q["V"] = [torch.stack([e["u"].expand(Q, H), g[:, None] * e["u"], e["d"].expand(Q, H)], 1).contiguous()
              for e, g in zip(pk["deep"], q["g"][1:])]                                 # [Q,3,64] per layer l >= 1
    q["vzero"] = torch.zeros((1, 3, H), device=E.device)
    pk["qcache"] = (key, q)
    return q


# rows of the post_mp tail per launch chain of a depth-L pass (its [rows, 256] intermediate is the largest buffer)
GOSSIP_DEEP_TAIL_ROWS = 1 << 24


def _gossip_deep_consts(batch: GossipBatch, x: torch.Tensor):
    """(C3 [R,3] = (deg_hi, deg_lo - deg_hi, 1), C4 [R,4] whose last column is 1) for x's number of query columns:
    functions of the CSR and that number alone, made on the first pass over a batch (eagerly: InferencePipeline.capture
    runs one first) and kept on it."""
    N, Q = x.shape
    cache = batch.__dict__.setdefault("_deep_consts", {})
    if Q not in cache:
        dev = x.device
        ones, zeros = torch.ones(Q, device=dev), torch.zeros(Q, device=dev)
        sa = ops.gossip_scalars(x, batch.rowptr, batch.col, ones, zeros)        # (deg_lo, s_lo, deg_hi, x)
        deg_lo, deg_hi = sa[:, 0], sa[:, 2]
        C3 = torch.stack([deg_hi, deg_lo - deg_hi, torch.ones_like(deg_hi)], 1).contiguous()
        cache[Q] = (C3, torch.ones((N * Q, 4), device=dev))
    return cache[Q]


def gossip_forward_deep(gnn: BaseGNN, batch: GossipBatch, query_emb: torch.Tensor) -> torch.Tensor:
    """Inference of a gossip model with L != 2 GossipConv layers: layer 0 in closed form
    (affine_rows), L - 1 launches of desco_gossip_layer_f16x3_f32 that also accumulate the h_l blocks of post_mp.0,
    then the post_mp tail.  The layer kernel takes any number of queries (the gates are per row); the per-row scalars
    of layer 0 (desco_gossip_scalars_f32) take at most 64, so more queries (--use_node_feature) go in column groups."""
    pk = gnn.packed()
    with torch.no_grad():
        q = _gossip_query_terms_deep(gnn, pk, query_emb)
    x = batch.x
    N, Q = x.shape
    if Q != query_emb.shape[0]:
        raise ValueError("batch.x has a different number of query columns than query_emb rows")
    if Q <= 64:
        return _gossip_deep_pass(gnn, pk, batch, x, q)
    outs = []
    for q0 in range(0, Q, 64):
        q1 = min(Q, q0 + 64)
        qs = {"g": [g[q0:q1].contiguous() for g in q["g"]], "V0": q["V0"][q0:q1].contiguous(),
              "Vacc": q["Vacc"][q0:q1].contiguous(), "V": [v[q0:q1].contiguous() for v in q["V"]], "vzero": q["vzero"]}
        outs.append(_gossip_deep_pass(gnn, pk, batch, x[:, q0:q1].contiguous(), qs))
    return torch.cat(outs, dim=1)


def _gossip_deep_pass(gnn: BaseGNN, pk: dict, batch: GossipBatch, x: torch.Tensor, q: dict) -> torch.Tensor:
    N, Q = x.shape
    L = gnn.gnn_core.layer_num
    C3, C4 = _gossip_deep_consts(batch, x)
    scal4 = ops.gossip_scalars(x, batch.rowptr, batch.col, q["g"][0], q["g"][0])    # (a0, b0, -, x)
    ops.copy2d_multi([(scal4[:, 0:2], C4[:, 0:2]), (scal4[:, 3:4], C4[:, 2:3])])   # C4 = (a0, b0, x, 1)
    h = ops.affine_rows(None, C4, q["V0"], ops.ACT_RELU, 0.0)                      # h1 (layer 0)
    acc = ops.affine_rows(None, C4, q["Vacc"], ops.ACT_NONE, 0.0)                  # zp + x tp
    if L == 1:
        ops.gemm_multi([dict(a1=h, wt=pk["p1t"], out=acc, accum=True)])
    for l in range(1, L):
        last = l == L - 1
        h = ops.gossip_layer_f16(h, batch.rowptr, batch.col, N, Q, q["g"][l], C3, q["V"][l - 1], pk["deep"][l - 1]["w"],
                                 pk["deep_p"][l - 1], acc, pn=pk["deep_p"][l] if last else None)
    del h
    (w3, b3), (w5, b5) = pk["post"]
    R = N * Q
    xf = x.reshape(-1)
    out = torch.empty((R,), device=x.device)
    for r0 in range(0, R, GOSSIP_DEEP_TAIL_ROWS):
        r1 = min(R, r0 + GOSSIP_DEEP_TAIL_ROWS)
        y = ops.affine_rows(acc[r0:r1], C3[r0:r1], q["vzero"], ops.ACT_LEAKY, 0.1)   # post_mp.2 (LeakyReLU 0.1)
        y = ops.gemm(y, w3, b3, act=ops.ACT_RELU)
        y = ops.gemm(y, w5, b5, act=ops.ACT_RELU)
        ops.rowdot_add(y, pk["w7"], pk["b7"], add=xf[r0:r1], out=out[r0:r1])          # post_mp.7 + x
        del y
    return out.view(N, Q)


def _gossip_query_terms(gnn: BaseGNN, pk: dict, query_emb: torch.Tensor) -> dict:
    """Everything that depends on (weights, query embeddings) only: gates and folded vectors."""
    key = (query_emb.data_ptr(), query_emb._version, tuple(query_emb.shape))
    if pk["qcache"] is not None and pk["qcache"][0] == key:
        return pk["qcache"][1]
    (g0, g1), *terms = _gossip_layer0_terms(gnn.gnn_core, gnn.post_mp[0], query_emb.float(), pk["w_pre"], pk["b_pre"])
    q = dict(zip(("p", "r", "t", "z", "tp", "zp"), (v.contiguous() for v in terms)))
    q["g0"], q["g1"] = g0.contiguous(), g1.contiguous()
    if "wstream" in pk:
        # the planned kernel's packed operands: [Q, 192] = p | z | zp, and the kernel's constant image + 1 / scales
        (_, b3), (_, b5) = pk["post"]
        q["pzz"] = torch.cat([q["p"], q["z"], q["zp"]], 1).contiguous()
        q["cst"] = torch.cat([pk["u1"], pk["d1"], q["tp"], b3, b5, pk["w7"], q["r"], q["t"], pk["winv"]]).contiguous()
    pk["qcache"] = (key, q)
    return q


# The planned kernel holds a node's first four neighbours in its plan record; further ones it reads in every query from
# the record and col again, where the unplanned kernel stages 15 columns per work unit in LDS.  Its measured gain is on
# molecule shapes (largest degree 4); batches in which more than this share of the nodes has more than four neighbours
# keep the unplanned launch -- exactly the launches from before the switch.  (The tile order sorts a tile's rows by degree,
# so the share of nodes is also about the share of 16-node groups that run the loop beyond four.)
GOSSIP_PLAN_LONG_ROW_SHARE = 1.0 / 16.0


def gossip_takes_plan(gnn: BaseGNN, batch: GossipBatch, num_q: int, tiled: bool = True) -> bool:
    """whether ``gossip_forward`` launches the planned kernel for a column group of ``num_q`` queries of ``batch``: the
    two-layer f16x3 pass, the switch on, the kernel's 32-bit bound kept, few rows beyond four neighbours.  The one place
    that decides it: the pipeline builds a batch's plan only where this holds."""
    return (GOSSIP_F16X3 and GOSSIP_PLAN and gnn.gnn_core.layer_num == 2 and batch.num_nodes > 0
            and batch.device.type == "cuda" and ops.gossip_plan_fits(batch.num_nodes, num_q, tiled)
            and batch.long_row_share <= GOSSIP_PLAN_LONG_ROW_SHARE)


def gossip_forward(gnn: BaseGNN, batch: GossipBatch, query_emb: torch.Tensor) -> torch.Tensor:
    """All-queries gossip correction + residual: returns pred [N, Q] = x + post_mp(emb)
    (BaseGNN.forward gossip path gnn_model.py:58-103 looped over queries as in
    lightning_model.py:613-628, here batched over the query axis)."""
    if gnn.gnn_core.layer_num != 2:
        return gossip_forward_deep(gnn, batch, query_emb)
    pk = gnn.packed()
    with torch.no_grad():
        q = _gossip_query_terms(gnn, pk, query_emb)
    x = batch.x
    N, Q = x.shape
    if Q != query_emb.shape[0]:
        raise ValueError("batch.x has a different number of query columns than query_emb rows")
    (w3, b3), (w5, b5) = pk["post"]
    outs = []
    # the scalars pre-pass maps one lane to one query: more than 64 queries (the labelled queries
    # of --use_node_feature) go in column groups
    for q0 in range(0, Q, 64):
        q1 = min(q0 + 64, Q)
        sl = (lambda t: t) if (q0 == 0 and q1 == Q) else (lambda t: t[q0:q1].contiguous())
        xs = x if (q0 == 0 and q1 == Q) else x[:, q0:q1].contiguous()
        scal4 = ops.gossip_scalars(xs, batch.rowptr, batch.col, sl(q["g0"]), sl(q["g1"]))
        v = {"g1": sl(q["g1"]), "p": sl(q["p"]), "z": sl(q["z"]), "zp": sl(q["zp"]), "r": q["r"],
             "t": q["t"], "u": pk["u1"], "tp": q["tp"], "d1": pk["d1"],
             # the fused kernel takes n-major ([out, in]) weight blocks
             "w1s": pk["fused_w1s"], "wps": pk["fused_wps"], "w3s": pk["fused_w3s"], "b3": b3,
             "w5s": pk["fused_w5s"], "b5": b5, "w7": pk["w7"], "b7": pk["b7"]}
        tperm = batch.tile_perm if GOSSIP_TILE_ORDER else None
        dst = getattr(batch, "out_buf", None) if (q0 == 0 and q1 == Q) else None
        if gossip_takes_plan(gnn, batch, q1 - q0, tperm is not None):
            vp = {"g1": v["g1"], "pzz": sl(q["pzz"]), "cst": q["cst"], "wstream": pk["wstream"], "b7": pk["b7"]}
            outs.append(ops.gossip_planned_f16(scal4, batch.col, N, q1 - q0, vp, batch.work_queue,
                                               batch.gossip_plan(tperm is not None), tperm is not None, out=dst))
        elif GOSSIP_F16X3:
            v["wstream"], v["winv"] = pk["wstream"], pk["winv"]
            outs.append(ops.gossip_fused_f16(scal4, batch.rowptr, batch.col, N, q1 - q0, v, batch.work_queue,
                                             tile_perm=tperm,
                                             out=getattr(batch, "out_buf", None) if (q0 == 0 and q1 == Q) else None))
        else:
            outs.append(ops.gossip_fused(scal4, batch.rowptr, batch.col, N, q1 - q0, v, tile_perm=tperm))
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)


def gossip_forward_train(gnn: BaseGNN, batch: GossipBatch, query_emb: torch.Tensor) -> torch.Tensor:
    """Differentiable twin of ``gossip_forward`` (returns pred [N, Q] = x + correction).

    Same algebra as the fused kernel as autograd Functions whose forward and
    backward are C-ABI launches.  As in the reference, the layer-0 input is detached
    (gnn_model.py:236-240): ``pre_mp`` and the query embeddings receive no gradient."""
    from . import autograd as AG
    core = gnn.gnn_core
    He = gossip_emb_width(core)
    if core.layer_num < 1 or not core.input_pattern_emb or core.input_dim != 1:
        raise NotImplementedError("gossip training implements GossipConv layers with input_dim 1 and the query "
                                  "embedding as input")
    x = batch.x
    N, Q = x.shape
    dev = x.device
    E = query_emb.detach().float().to(dev)
    w_pre, b_pre = core.pre_mp[0].weight[:, 0].detach(), core.pre_mp[0].bias.detach()
    c0 = core.convs[0]
    C0, cb0, D0, db0 = c0.lin_com.weight, c0.lin_com.bias, c0.lin_update.weight, c0.lin_update.bias
    # ---- constants per (node, query): deg_lo, deg_hi, s_lo, s_hi, x (functions of the batch alone: cached on it) ----
    # (keyed on the tensor object -- kept alive by the cache, so its address cannot be reused -- and its version;
    #  the library's in-place writers of x bump the version: ops.scatter_rows)
    cc = batch.__dict__.get("_train_consts")
    if cc is None or cc[0][0] is not x or cc[0][1] != x._version:
        with torch.no_grad():
            ones, zeros = torch.ones(Q, device=dev), torch.zeros(Q, device=dev)
            sa = ops.gossip_scalars(x, batch.rowptr, batch.col, ones, zeros)    # (deg_lo, s_lo, deg_hi, x)
            sb = ops.gossip_scalars(x, batch.rowptr, batch.col, zeros, zeros)   # (deg_hi, s_hi, deg_hi, x)
            deg_lo, s_lo, deg_hi, xr = sa[:, 0], sa[:, 1], sa[:, 2], sa[:, 3]
            s_hi = sb[:, 1]
            one = torch.ones_like(xr)
            C6 = torch.stack([deg_hi, deg_lo - deg_hi, s_hi, s_lo - s_hi, xr, one], 1).contiguous()
            C3 = torch.stack([deg_hi, deg_lo - deg_hi, one], 1).contiguous()
            C2 = torch.stack([xr, one], 1).contiguous()
        cc = batch.__dict__["_train_consts"] = ((x, x._version), C6, C3, C2)
    _, C6, C3, C2 = cc
    # --gossip_dropout (default 0.01, config.py:316): F.dropout behind each layer's relu (gnn_model.py:274) and
    # post_mp.1 = nn.Dropout (:46), in training mode only -- counter-based factors inside GossipTrunk's epilogues
    p_layer = float(core.dropout or 0.0) if gnn.training else 0.0
    p_post = float(gnn.post_mp[1].p or 0.0) if gnn.training else 0.0
    drop = (p_layer, p_post) if (p_layer > 0.0 or p_post > 0.0 or (DROPOUT_AT_ZERO and gnn.training)) else None
    if core.layer_num != 2:
        return _gossip_train_deep(gnn, batch, E, w_pre, b_pre, C6, C3, C2, drop).view(N, Q)
    c1 = core.convs[1]
    C1, cb1, D1, db1 = c1.lin_com.weight, c1.lin_com.bias, c1.lin_update.weight, c1.lin_update.bias
    if Q <= 64 and He == H:
        # The operands folded from the parameters by one kernel each way (autograd.FoldGossip, csrc/train_native.hip;
        # algebra DESIGN.md 4.2), then the whole per-(node, query) pipeline and its backward as one autograd node
        # (autograd.GossipTrunk): the step launches nothing but this library's kernels.
        gl = [c.lin_gate for c in (c0, c1)]
        V0, g1, g1c, wt1, V1, wtp, Vp, w3t, w5t = AG.FoldGossip.apply(
            E.contiguous(), w_pre.contiguous(), b_pre.contiguous(), C0, cb0, D0, db0, C1, cb1, D1, db1,
            gl[0][0].weight, gl[0][0].bias, gl[0][2].weight, gl[0][2].bias,
            gl[1][0].weight, gl[1][0].bias, gl[1][2].weight, gl[1][2].bias,
            gnn.post_mp[0].weight, gnn.post_mp[0].bias, gnn.post_mp[3].weight, gnn.post_mp[5].weight)
        pred = AG.GossipTrunk.apply(batch.rowptr, batch.col, N, Q, C6, C3, C2, x.reshape(-1), g1c,
                                    gnn.post_mp[3].weight.detach(), gnn.post_mp[5].weight.detach(), drop,
                                    V0, g1, wt1, V1, wtp, Vp, w3t, gnn.post_mp[3].bias, w5t, gnn.post_mp[5].bias,
                                    gnn.post_mp[7].weight.view(-1), gnn.post_mp[7].bias)
        return pred.view(N, Q)
    # ---- operands folded from the parameters with differentiable torch ops (more than 64 queries, or query embeddings
    #      of another width than 64) -------------------------------------------------------------------------------------
    (g0, g1), p, r, t, z, tp, zp = _gossip_layer0_terms(core, gnn.post_mp[0], E, w_pre, b_pre)
    r, t = r.expand(Q, H), t.expand(Q, H)
    V0 = torch.stack([p, g0[:, None] * p, r, g0[:, None] * r, t, z], 1)          # [Q,6,64]
    D1a, D1b = D1[:, :H], D1[:, H:]
    wt1 = torch.cat([(D1a @ C1).t(), D1b.t()], 0)
    u = _mv(D1a, cb1).expand(Q, H)
    V1 = torch.stack([u, g1[:, None] * u, db1.expand(Q, H)], 1)                     # [Q,3,64]
    P0 = gnn.post_mp[0].weight
    wtp = torch.cat([P0[:, He + H:He + 2 * H].t(), P0[:, He + 2 * H:He + 3 * H].t()], 0)
    Vp = torch.stack([tp.expand(Q, H), zp], 1)                                      # [Q,2,64]
    pred = AG.GossipTrunk.apply(batch.rowptr, batch.col, N, Q, C6, C3, C2, x.reshape(-1), (1.0 - g1).detach().contiguous(),
                                gnn.post_mp[3].weight.detach(), gnn.post_mp[5].weight.detach(), drop,
                                V0, g1, wt1, V1, wtp, Vp, gnn.post_mp[3].weight.t(), gnn.post_mp[3].bias,
                                gnn.post_mp[5].weight.t(), gnn.post_mp[5].bias, gnn.post_mp[7].weight.view(-1),
                                gnn.post_mp[7].bias)
    return pred.view(N, Q)


def _gossip_train_deep(gnn: BaseGNN, batch: GossipBatch, E, w_pre, b_pre, C6, C3, C2, drop) -> torch.Tensor:
    """Training pass of a depth-L model (L != 2): the operands folded from the parameters with differentiable torch ops
    (the form of the more-than-64-queries branch, per layer), then autograd.GossipTrunkDeep."""
    from . import autograd as AG
    core = gnn.gnn_core
    He = gossip_emb_width(core)
    L = core.layer_num
    x = batch.x
    N, Q = x.shape
    g, p, r, t, z, tp, zp = _gossip_layer0_terms(core, gnn.post_mp[0], E, w_pre, b_pre)
    r, t = r.expand(Q, H), t.expand(Q, H)
    V0 = torch.stack([p, g[0][:, None] * p, r, g[0][:, None] * r, t, z], 1)      # [Q,6,64]
    lw = []
    for l in range(1, L):
        c = core.convs[l]
        Da, Db = c.lin_update.weight[:, :H], c.lin_update.weight[:, H:]
        u = _mv(Da, c.lin_com.bias).expand(Q, H)
        lw += [g[l], torch.cat([(Da @ c.lin_com.weight).t(), Db.t()], 0),
               torch.stack([u, g[l][:, None] * u, c.lin_update.bias.expand(Q, H)], 1)]
    P0 = gnn.post_mp[0].weight
    wtp = torch.cat([P0[:, He + l * H:He + (l + 1) * H].t() for l in range(1, L + 1)], 0)   # [64 L, 64]
    Vp = torch.stack([tp.expand(Q, H), zp], 1)                                      # [Q,2,64]
    return AG.GossipTrunkDeep.apply(batch.rowptr, batch.col, N, Q, C6, C3, C2, x.reshape(-1),
                                    gnn.post_mp[3].weight.detach(), gnn.post_mp[5].weight.detach(), drop, L,
                                    V0, gnn.post_mp[3].weight.t(), gnn.post_mp[3].bias, gnn.post_mp[5].weight.t(),
                                    gnn.post_mp[5].bias, gnn.post_mp[7].weight.view(-1), gnn.post_mp[7].bias, wtp, Vp,
                                    *lw)
