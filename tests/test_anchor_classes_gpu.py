"""gnn_model.ANCHOR_CLASS_TABLE: the anchor MLP on one representative per class of anchor operands
(NeighborhoodBatch.anchor_class_index), post_mp.0 reading the anchor rows through the classes
(desco_pool_post_rows_bf16x6_f32) in place of the one-launch anchor + post_mp.0 (desco_anchor_pool_post_f16x3_f32).
Everything is a bit-for-bit comparison (torch.equal) of the pass with the switch on against the pass with the switch off; the
premise -- neighborhoods of one class have bit-equal anchor operands and row bounds -- is checked on the operand the
switched-off pass hands to its launch, not assumed.

gnn_model.CANON_CLASS_TABLES on top of it: the canonical rows of every layer as tables of their distinct rows
(NeighborhoodBatch.canonical_class_tables), the canonical launches on one representative per class, the anchor operand's U_a
rows and their bounds gathered from the tables -- compared bit for bit with the rows the path above gathers from the [B, .]
operand.

The pass takes the path on blocks of at least NeighborhoodBatch.ANCHOR_CLASS_MIN_ROWS neighborhoods (a bound on the profit);
the small blocks here lower it and the other profit bounds on their own batch object, and set the depth they test."""
from collections import Counter

import pytest
import torch

pytestmark = pytest.mark.gpu

import desco_amd.gnn_model as GM  # noqa: E402
from desco_amd import ops, synthetic  # noqa: E402
from desco_amd.batch import NeighborhoodBatch  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402
from desco_amd.partition import build_partition  # noqa: E402

from helpers import make_models, neigh_args, standard_queries  # noqa: E402

DEV = "cuda"
FUSED = "anchor_pool_post_kernel"
F16X3 = "gemm_f16x3_kernel"


def _model(layer_num):
    if layer_num == 8:
        nm, _ = make_models(seed=0)
    else:
        from desco_amd.lightning_model import NeighborhoodCountingModel
        torch.manual_seed(layer_num)
        nm = NeighborhoodCountingModel(1, 64, neigh_args(layer_num=layer_num)).to_hetero_old(True, True)
        with torch.no_grad():          # (default init lets the relu layers collapse: widen the matrices, as make_models does)
            for w in nm.parameters():
                if w.dim() == 2:
                    w.mul_(1.3)
    nm = nm.to(DEV)
    nm.set_queries(standard_queries()[0])
    return nm


@pytest.fixture(scope="module")
def models():
    return {L: _model(L) for L in (8, 5)}


def _lower(b, max_level=8, anchor=True):
    b.LAYER2_MIN_ROWS_PER_CLASS = b.LAYER3_MIN_ROWS_PER_CLASS = b.DEEP_TABLE_MIN_ROWS_PER_CLASS = 1
    b.LAYER2_GATHER_MIN_ROWS = b.LAYER3_MIN_ROWS = b.POOL_TABLES_MIN_ROWS = b.DEEP_TABLE_MIN_ROWS = 0
    b.DEEP_TABLE_MAX_LEVEL = max_level
    if anchor:
        b.ANCHOR_CLASS_MIN_ROWS, b.ANCHOR_CLASS_MIN_ROWS_PER_CLASS = 0, 1
    return b


def _batch(graphs, max_level=8, anchor=True):
    gs = graphs if isinstance(graphs, GraphSet) else GraphSet.from_edge_lists(graphs)
    return _lower(NeighborhoodBatch(build_partition(gs, 4), DEV), max_level, anchor)


def _pass(nm, batch, on, deep=True, canon=False):
    """(logits, kernel names, rows of the f16x3 GEMM launches, the (anchor operand, row bound) handed to the one-launch anchor +
    post_mp.0, the (table rows, ids) of the pool_post launches) of one inference pass with ANCHOR_CLASS_TABLE = ``on``,
    DEEP_LAYER_TABLES = ``deep`` and CANON_CLASS_TABLES = ``canon``; the (operand, row bound) of the f16x3 GEMM launches and the
    launch rows of the layer launches are left in ``_pass.operands`` / ``_pass.layer_rows``"""
    gemms, fused, posts = [], [], []
    _pass.operands, _pass.layer_rows = [], []
    real = ops.gemm_f16x3, ops.anchor_pool_post, ops.pool_post, ops.shmp_layer

    def spy_gemm(a1, *a, **kw):
        gemms.append(a1.shape[0])
        _pass.operands.append((a1.clone(), None if kw.get("row_scale") is None else kw["row_scale"].clone()))
        return real[0](a1, *a, **kw)

    def spy_layer(x, vrowptr, vcol, row0, num_rows, *a, **kw):
        _pass.layer_rows.append(num_rows)
        return real[3](x, vrowptr, vcol, row0, num_rows, *a, **kw)

    def spy_fused(a, anchor_w, anchor_bias, row_scale, *r, **kw):
        fused.append((a.clone(), row_scale.clone()))
        return real[1](a, anchor_w, anchor_bias, row_scale, *r, **kw)

    def spy_post(anch, *a, **kw):
        ids = kw.get("anch_row")
        posts.append((anch.shape[0], None if ids is None else ids.numel()))
        return real[2](anch, *a, **kw)

    old = GM.ANCHOR_CLASS_TABLE, GM.DEEP_LAYER_TABLES, GM.CANON_CLASS_TABLES
    GM.ANCHOR_CLASS_TABLE, GM.DEEP_LAYER_TABLES, GM.CANON_CLASS_TABLES = on, deep, canon
    ops.gemm_f16x3, ops.anchor_pool_post, ops.pool_post, ops.shmp_layer = spy_gemm, spy_fused, spy_post, spy_layer
    ops.PROFILER.reset()
    ops.PROFILER.enabled = True
    try:
        out = nm.graph_to_count(batch).clone()
        torch.cuda.synchronize()
        names = [r[0] for r in ops.PROFILER.records]
    finally:
        GM.ANCHOR_CLASS_TABLE, GM.DEEP_LAYER_TABLES, GM.CANON_CLASS_TABLES = old
        ops.gemm_f16x3, ops.anchor_pool_post, ops.pool_post, ops.shmp_layer = real
        ops.PROFILER.enabled = False
        ops.PROFILER.reset()
    return out, names, gemms, fused, posts


GRAPHS = {"mutag24": lambda: synthetic.mutag_shaped(24), "cox2 cut": lambda: synthetic.cox2_shaped(12)}


@pytest.mark.parametrize("layers", [8, 5])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_eligible_batch_takes_the_path_and_changes_no_bit(models, name, layers):
    nm, batch = models[layers], _batch(GRAPHS[name](), max_level=layers)
    if name == "mutag24":
        assert batch.num_count == 2795
    B = batch.num_graphs
    assert len(batch.deep_table_index()) == layers - 3
    acls, arep = batch.anchor_class_index(layers)
    ua = arep.numel()
    assert acls.shape == (B,) and 1 < ua < B and int(acls.max()) == ua - 1 and int(arep.max()) < B
    nm.graph_to_count(batch)                 # (the first pass of a model also folds and splits its weights)
    on, names_on, gemms_on, fused_on, posts_on = _pass(nm, batch, True)
    operands_on, layer_rows_on = _pass.operands, _pass.layer_rows
    off, names_off, gemms_off, fused_off, posts_off = _pass(nm, batch, False)
    assert torch.isfinite(on).all() and torch.equal(on, off)
    # the premise: every neighborhood's anchor operand and row bound are its class representative's, bit for bit
    (canon, bound), = fused_off
    rep = arep[acls.long()]
    assert canon.shape == (B, 64 * layers) and torch.equal(canon, canon[rep]) and torch.equal(bound, bound[rep])
    assert torch.unique(canon, dim=0).shape[0] <= ua                       # (no more distinct operands than classes)
    # the switched-off pass is the one-launch form; the path: no such launch, one f16x3 GEMM on U_a rows, post_mp.0 through ids
    assert names_off.count(FUSED) == 1 and not fused_on and FUSED not in names_on
    assert ua not in gemms_off and gemms_on.count(ua) == 1 and sorted(gemms_on) == sorted(gemms_off + [ua])
    assert names_on.count(F16X3) == names_off.count(F16X3) + 1
    assert posts_on == [(ua, B)] and posts_off == []
    # nothing else of the pass changes: the same launches besides (the gathers are torch's)
    assert sorted(names_on) == sorted([k for k in names_off if k != FUSED] + [F16X3, "gemm_split_kernel"])
    # its GEMM's operand and row bound: the representatives' rows of the operand the switched-off pass hands over
    (a_on, bound_on), = [o for o in operands_on if o[0].shape[0] == ua]
    assert torch.equal(a_on, canon[arep]) and torch.equal(bound_on, bound[arep])
    assert layer_rows_on == _pass.layer_rows and layer_rows_on.count(B) == layers - 1                            # (the canonical launches on every neighborhood)

    # CANON_CLASS_TABLES: the same logits, the same operand and bound for the anchor GEMM -- gathered from the tables
    tabs = batch.canonical_class_tables(layers)
    assert tabs is not None and tabs.size[-1] == ua and not {B, batch.num_count} & set(tabs.size)
    both, names_both, gemms_both, fused_both, posts_both = _pass(nm, batch, True, canon=True)
    assert torch.isfinite(both).all() and torch.equal(both, off)
    (a_both, bound_both), = [o for o in _pass.operands if o[0].shape[0] == ua]
    assert torch.equal(a_both, a_on) and torch.equal(bound_both, bound_on)
    assert not fused_both and FUSED not in names_both and posts_both == [(ua, B)] and gemms_both == gemms_on
    # no layer launch on the n - nc canonical rows: one per level on the classes' representatives instead, in order
    assert B not in _pass.layer_rows and len(_pass.layer_rows) == len(layer_rows_on)
    assert Counter(_pass.layer_rows) - Counter(layer_rows_on) == Counter(tabs.size[1:])
    assert Counter(layer_rows_on) - Counter(_pass.layer_rows) == Counter({B: layers - 1})
    # the table products of the levels read the canonical tables as they are: no launch besides the project's own changes
    assert names_both.count(F16X3) == names_on.count(F16X3) and names_both.count("linear64_kernel") == names_on.count("linear64_kernel")


@pytest.mark.parametrize("name", ["new bounds at their defaults", "rows per class", "deep tables off", "K < L", "K > L"])
def test_ineligible_batch_launches_the_parents_kernels(models, name):
    nm = models[8]
    g = synthetic.mutag_shaped(24)
    deep = True
    if name == "new bounds at their defaults":           # every older bound lowered, as the older tests lower them
        batch = _batch(g, anchor=False)
        assert batch.ANCHOR_CLASS_MIN_ROWS == NeighborhoodBatch.ANCHOR_CLASS_MIN_ROWS >= 1 << 20
        assert batch.ANCHOR_CLASS_MIN_ROWS_PER_CLASS == NeighborhoodBatch.ANCHOR_CLASS_MIN_ROWS_PER_CLASS == 8
    elif name == "rows per class":
        batch = _batch(g)
        batch.ANCHOR_CLASS_MIN_ROWS_PER_CLASS = batch.num_graphs
    elif name == "deep tables off":
        batch, deep = _batch(g), False
    elif name == "K < L":
        batch = _batch(g, max_level=6)
    else:
        nm, batch = models[5], _batch(g, max_level=8)
    if name not in ("deep tables off",):
        assert batch.anchor_class_index(8 if name != "K > L" else 5) is None
    nm.graph_to_count(batch)
    on, names_on, gemms_on, fused_on, posts_on = _pass(nm, batch, True, deep, canon=True)
    off, names_off, gemms_off, fused_off, posts_off = _pass(nm, batch, False, deep)
    assert names_on == names_off and names_on.count(FUSED) == 1 and gemms_on == gemms_off and posts_on == posts_off == []
    assert len(fused_on) == 1 and torch.equal(fused_on[0][0], fused_off[0][0])
    assert torch.isfinite(on).all() and torch.equal(on, off)


KEYS = ("neigh_count", "node_count", "graph_neigh_count", "graph_gossip_count")


def test_pipeline_outputs_are_equal_and_a_captured_replay_equals_the_eager_pass():
    from desco_amd.pipeline import InferencePipeline
    nm, gm = make_models(seed=0)
    nm, gm = nm.to(DEV), gm.to(DEV)
    nm.set_queries(standard_queries()[0])
    pipe = InferencePipeline(nm, gm, synthetic.mutag_shaped(188), depth=4, device=DEV)
    for b in pipe.neigh_batches:
        _lower(b)
    assert all(b.anchor_class_index(8) is not None for b in pipe.neigh_batches)
    pipe.run()                               # (the first pass of a model also folds and splits its weights)
    old = GM.ANCHOR_CLASS_TABLE, GM.CANON_CLASS_TABLES
    res = {}
    try:
        for on in ("both", True, False):
            GM.ANCHOR_CLASS_TABLE, GM.CANON_CLASS_TABLES = bool(on), on == "both"
            ops.PROFILER.reset()
            ops.PROFILER.enabled = True
            res[on] = {k: v.clone() for k, v in pipe.run().items() if k in KEYS}
            torch.cuda.synchronize()
            res[on]["fused"] = [r[0] for r in ops.PROFILER.records].count(FUSED)
            ops.PROFILER.enabled = False
        GM.ANCHOR_CLASS_TABLE = GM.CANON_CLASS_TABLES = True
        pipe.capture()
        rep = pipe.run_graph()
        torch.cuda.synchronize()
    finally:
        GM.ANCHOR_CLASS_TABLE, GM.CANON_CLASS_TABLES = old
        ops.PROFILER.enabled = False
        ops.PROFILER.reset()
    assert res["both"]["fused"] == res[True]["fused"] == 0 and res[False]["fused"] == len(pipe.neigh_batches)
    for k in KEYS:
        assert torch.isfinite(res[True][k]).all() and torch.equal(res[True][k], res[False][k]), k
        assert torch.equal(res["both"][k], res[False][k]) and torch.equal(res["both"][k], rep[k]), k
