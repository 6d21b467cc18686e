"""gnn_model.POOL_CLASS_TABLE: the pooled sums, post_mp and the count head on one representative per pooling class
(NeighborhoodBatch.pool_class_index; desco_class_rows_pool_f32 in place of the walk over every count row), the counts handed
out by one gather (desco_gather_rows_f32).  Everything is a bit-for-bit comparison (torch.equal) of the pass with the switch
on against the pass with the switch off.

The pass takes the path on blocks of at least NeighborhoodBatch.POOL_CLASS_MIN_ROWS neighborhoods (a bound on the profit); the
small blocks here lower it and the other profit bounds on their own batch object, and set the depth they test."""
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
WALK, CLASS_ROWS, GATHER = "table_rows_pool_kernel", "class_rows_pool_kernel", "gather_rows_kernel"


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


def _lower(b, max_level=8, pool=True):
    b.LAYER2_MIN_ROWS_PER_CLASS = b.LAYER3_MIN_ROWS_PER_CLASS = b.DEEP_TABLE_MIN_ROWS_PER_CLASS = 1
    b.LAYER2_GATHER_MIN_ROWS = b.LAYER3_MIN_ROWS = b.POOL_TABLES_MIN_ROWS = b.DEEP_TABLE_MIN_ROWS = 0
    b.DEEP_TABLE_MAX_LEVEL = max_level
    b.ANCHOR_CLASS_MIN_ROWS, b.ANCHOR_CLASS_MIN_ROWS_PER_CLASS = 0, 1
    if pool:
        b.POOL_CLASS_MIN_ROWS, b.POOL_CLASS_MIN_ROWS_PER_CLASS = 0, 1
    return b


def _batch(graphs, max_level=8, pool=True):
    gs = graphs if isinstance(graphs, GraphSet) else GraphSet.from_edge_lists(graphs)
    return _lower(NeighborhoodBatch(build_partition(gs, 4), DEV), max_level, pool)


def _pass(nm, batch, on):
    """(counts, logits, kernel names of the counts' pass) of inference passes with POOL_CLASS_TABLE = ``on``"""
    old = GM.POOL_CLASS_TABLE
    GM.POOL_CLASS_TABLE = on
    ops.PROFILER.reset()
    ops.PROFILER.enabled = True
    try:
        counts = nm.graph_to_count(batch).clone()
        torch.cuda.synchronize()
        names = [r[0] for r in ops.PROFILER.records]
        ops.PROFILER.enabled = False
        with torch.no_grad():
            logits = nm._logits(batch, exp2=False).clone()
    finally:
        GM.POOL_CLASS_TABLE = old
        ops.PROFILER.enabled = False
        ops.PROFILER.reset()
    return counts, logits, names


GRAPHS = {"mutag24": lambda: synthetic.mutag_shaped(24), "cox2 cut": lambda: synthetic.cox2_shaped(12)}


@pytest.mark.parametrize("layers", [8, 5])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_eligible_batch_takes_the_path_and_changes_no_bit(models, name, layers):
    nm, batch = models[layers], _batch(GRAPHS[name](), max_level=layers)
    B = batch.num_graphs
    pcls, prep = batch.pool_class_index(layers)
    up = prep.numel()
    assert pcls.shape == (B,) and 1 < up <= B and int(pcls.max()) == up - 1 and int(prep.max()) < B
    nm.graph_to_count(batch)                 # (the first pass of a model also folds and splits its weights)
    on, logits_on, names_on = _pass(nm, batch, True)
    off, logits_off, names_off = _pass(nm, batch, False)
    assert on.shape == (B, 29) and torch.isfinite(on).all() and torch.equal(on, off)
    assert torch.isfinite(logits_on).all() and torch.equal(logits_on, logits_off)
    # no walk over the count rows, the representatives' sums and the gather once each; nothing else of the pass changes
    assert WALK in names_off and CLASS_ROWS not in names_off and GATHER not in names_off
    assert WALK not in names_on and names_on.count(CLASS_ROWS) == 1 and names_on.count(GATHER) == 1
    assert sorted(names_on) == sorted([k for k in names_off if k != WALK] + [CLASS_ROWS, GATHER])
    # the embeddings, too: gathered for callers that want one row per neighborhood
    old = GM.POOL_CLASS_TABLE
    try:
        GM.POOL_CLASS_TABLE = True
        emb_on = nm.graph_to_embed(batch)
        GM.POOL_CLASS_TABLE = False
        emb_off = nm.graph_to_embed(batch)
    finally:
        GM.POOL_CLASS_TABLE = old
    assert emb_on.shape == (B, 64) and torch.equal(emb_on, emb_off)


def test_the_parents_launches_hold_at_the_default_bounds(models):
    nm, batch = models[8], _batch(synthetic.mutag_shaped(24), pool=False)
    assert batch.POOL_CLASS_MIN_ROWS == NeighborhoodBatch.POOL_CLASS_MIN_ROWS >= 1 << 20
    assert batch.POOL_CLASS_MIN_ROWS_PER_CLASS == NeighborhoodBatch.POOL_CLASS_MIN_ROWS_PER_CLASS == 8
    assert batch.anchor_class_index(8) is not None and batch.pool_class_index(8) is None
    nm.graph_to_count(batch)
    on, logits_on, names_on = _pass(nm, batch, True)
    off, logits_off, names_off = _pass(nm, batch, False)
    assert names_on == names_off and WALK in names_on and CLASS_ROWS not in names_on and GATHER not in names_on
    assert torch.equal(on, off) and torch.equal(logits_on, logits_off)
    # ... and with the rows-per-class bound alone at its default
    batch = _batch(synthetic.mutag_shaped(24))
    batch.POOL_CLASS_MIN_ROWS_PER_CLASS = 8
    assert batch.pool_class_index(8) is None
    assert _pass(nm, batch, True)[2] == names_off


def test_every_neighborhood_its_own_class(models):
    # the finest partition there is: the identity index in place of the batch's own (a refinement of it, so still exact)
    nm, batch = models[8], _batch(synthetic.mutag_shaped(24))
    B = batch.num_graphs
    batch.__dict__["_pool_class"] = {8: (torch.arange(B, dtype=torch.int32, device=DEV), torch.arange(B, device=DEV))}
    assert batch.pool_class_launch_index(8).prep.numel() == B
    nm.graph_to_count(batch)
    on, logits_on, names_on = _pass(nm, batch, True)
    off, logits_off, _ = _pass(nm, batch, False)
    assert names_on.count(CLASS_ROWS) == 1 and torch.equal(on, off) and torch.equal(logits_on, logits_off)


KEYS = ("neigh_count", "node_count", "graph_neigh_count", "graph_gossip_count")


def test_pipeline_outputs_are_equal_and_a_captured_replay_equals_the_eager_pass():
    from desco_amd.pipeline import InferencePipeline
    nm, gm = make_models(seed=0)
    nm, gm = nm.to(DEV), gm.to(DEV)
    nm.set_queries(standard_queries()[0])
    pipe = InferencePipeline(nm, gm, synthetic.mutag_shaped(188), depth=4, device=DEV)
    for b in pipe.neigh_batches:
        _lower(b)
    assert all(b.pool_class_index(8) is not None for b in pipe.neigh_batches)
    pipe.run()                               # (the first pass of a model also folds and splits its weights)
    old = GM.POOL_CLASS_TABLE
    res = {}
    try:
        for on in (True, False):
            GM.POOL_CLASS_TABLE = on
            ops.PROFILER.reset()
            ops.PROFILER.enabled = True
            res[on] = {k: v.clone() for k, v in pipe.run().items() if k in KEYS}
            torch.cuda.synchronize()
            res[on]["class"] = [r[0] for r in ops.PROFILER.records].count(CLASS_ROWS)
            ops.PROFILER.enabled = False
        GM.POOL_CLASS_TABLE = True
        pipe.capture()
        rep = pipe.run_graph()
        torch.cuda.synchronize()
    finally:
        GM.POOL_CLASS_TABLE = old
        ops.PROFILER.enabled = False
        ops.PROFILER.reset()
    assert res[True]["class"] == len(pipe.neigh_batches) and res[False]["class"] == 0
    for k in KEYS:
        assert torch.isfinite(res[True][k]).all() and torch.equal(res[True][k], res[False][k]), k
        assert torch.equal(rep[k], res[False][k]), k
