"""gnn_model.THIRD_LAYER_TABLE: the third SHMP layer's count launch on one representative per class of its output
(NeighborhoodBatch.layer3_table_index), X_3's count rows never written, the fourth layer gathering from the table, the partial
sums of the three table layers from one walk.  Everything is a bit-for-bit comparison (torch.equal) of the pass with the switch
on against the pass with the switch off: the layer kernel's arithmetic is row-local and, with at most 8 sources per row, its
gather order a function of the row alone.

The pass takes the path on blocks of at least NeighborhoodBatch.LAYER3_MIN_ROWS count rows with at least 8 rows per class
(bounds on the profit); the small blocks here lower them on their own batch object, with the LAYER2_* bounds."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import desco_amd.gnn_model as GM  # noqa: E402
from desco_amd import ops, synthetic  # noqa: E402
from desco_amd.batch import NeighborhoodBatch  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402
from desco_amd.partition import build_partition  # noqa: E402

from helpers import golden_graphs, make_models, neigh_args, standard_queries  # noqa: E402

DEV = "cuda"
PLAIN = "shmp_layer16_kernel<3,2,f16x3>"
SELFIDX = "shmp_layer16_kernel<3,2,f16x3,selfidx>"
WALK = "table_rows_pool_kernel"


def _path(n):
    return (n, [(i, i + 1) for i in range(n - 1)])


def _ring(n):
    return (n, [(i, (i + 1) % n) for i in range(n)])


def _star(k):
    return (k + 1, [(0, v) for v in range(1, k + 1)])


SMALL = ([_path(n) for n in range(2, 8)] + [_ring(5), _ring(6)] + [_star(k) for k in range(1, 5)]) * 3


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
    return {L: _model(L) for L in (8, 4, 3)}


def _lower(b, pool_tables=True):
    b.LAYER2_MIN_ROWS_PER_CLASS = b.LAYER3_MIN_ROWS_PER_CLASS = 1
    b.LAYER2_GATHER_MIN_ROWS = b.LAYER3_MIN_ROWS = 0
    if pool_tables:
        b.POOL_TABLES_MIN_ROWS = 0
    return b


def _batch(graphs, lowered=True, pool_tables=True):
    gs = graphs if isinstance(graphs, GraphSet) else GraphSet.from_edge_lists(graphs)
    b = NeighborhoodBatch(build_partition(gs, 4), DEV)
    return _lower(b, pool_tables) if lowered else b


def _pass(nm, batch, on):
    """(logits, kernel names, the layer launches (rows of x, launch rows, rows of out or None, self index given), the rows of
    the linear64 launches, the table walks (out, entries of ``pool``)) of one inference pass"""
    layers, products, walks = [], [], []
    real = ops.shmp_layer, ops.linear64, ops.table_rows_pool

    def spy_layer(x, vrowptr, vcol, row0, num_rows, *a, **kw):
        out = a[4] if len(a) > 4 else kw.get("out")
        layers.append((x.shape[0], num_rows, None if out is None else out.shape[0], kw.get("self_index") is not None))
        return real[0](x, vrowptr, vcol, row0, num_rows, *a, **kw)

    def spy_linear(x, *a, **kw):
        products.append(x.shape[0])
        return real[1](x, *a, **kw)

    def spy_walk(table, cls, n, out, pool):
        walks.append((out, len(pool)))
        real[2](table, cls, n, out, pool)

    old = GM.THIRD_LAYER_TABLE
    GM.THIRD_LAYER_TABLE = on
    ops.shmp_layer, ops.linear64, ops.table_rows_pool = spy_layer, spy_linear, spy_walk
    ops.PROFILER.reset()
    ops.PROFILER.enabled = True
    try:
        out = nm.graph_to_count(batch).clone()
        torch.cuda.synchronize()
        names = [r[0] for r in ops.PROFILER.records]
    finally:
        GM.THIRD_LAYER_TABLE = old
        ops.shmp_layer, ops.linear64, ops.table_rows_pool = real
        ops.PROFILER.enabled = False
        ops.PROFILER.reset()
    return out, names, layers, products, walks


def _renamed(names_on, names_off, layers):
    """the parent's launches but: the walk behind the third layer's count launch, and (a fourth layer) its count launch under
    the SELFIDX name"""
    a, b = [n for n in names_on if n != WALK], [n for n in names_off if n != WALK]
    diff = [(x, y) for x, y in zip(a, b) if x != y]
    return (len(a) == len(b) and names_on.count(WALK) == names_off.count(WALK) == 1
            and diff == ([(SELFIDX, PLAIN)] if layers >= 4 else []) and names_on.index(WALK) > names_off.index(WALK))


ELIGIBLE = {"mutag24": lambda **kw: _batch(synthetic.mutag_shaped(24), **kw), "small": lambda **kw: _batch(SMALL, **kw),
            "cox2 cut": lambda **kw: _batch(synthetic.cox2_shaped(12), **kw)}


@pytest.mark.parametrize("layers", [8, 4, 3])
@pytest.mark.parametrize("pool_tables", [True, False], ids=["three-table walk", "two-table walk"])
@pytest.mark.parametrize("name", list(ELIGIBLE))
def test_eligible_batch_takes_the_path_and_changes_no_bit(models, name, layers, pool_tables):
    nm, batch = models[layers], ELIGIBLE[name](pool_tables=pool_tables)
    assert batch.num_count < 6000
    tab3 = batch.layer3_table_index()
    assert tab3 is not None
    u2, u3, uc2 = (batch.layer2_table_index()[1].numel() - 1) // 4, tab3[3].numel(), tab3[6].numel()
    nc, n = batch.num_count, batch.num_rows
    assert len({u2, u3, uc2, nc, n, batch.num_graphs}) == 6             # (so that a launch is known by its row counts)
    nm.graph_to_count(batch)                 # (the first pass of a model also folds and splits its weights)
    on, names_on, layers_on, products_on, walks_on = _pass(nm, batch, True)
    off, names_off, layers_off, products_off, walks_off = _pass(nm, batch, False)
    assert torch.isfinite(on).all() and torch.equal(on, off)
    # no [N, 64] output for layer 3: the launches that read table2 write the representatives' rows or (canonical) none
    third = [c for c in layers_on if c[0] == u2]
    assert sorted(third) == sorted([(u2, u3, u3, True), (u2, n - nc, None, False)])
    assert [c for c in layers_on if c[1] == u3] == [(u2, u3, u3, True)]             # exactly one count launch on U_3 rows
    assert (u2, nc, None if layers == 3 else n, True) in layers_off                 # (the parent: on every count row)
    # the fourth layer's launches gather from table3, the count launch with its own rows through cls3
    fourth = [c for c in layers_on if c[0] == u3]
    assert sorted(fourth) == (sorted([(u3, nc, None if layers == 4 else n, True), (u3, n - nc, None, False)]) if layers >= 4 else [])
    assert names_on.count(SELFIDX) == (2 if layers >= 4 else 1) and names_off.count(SELFIDX) == 1
    assert products_on.count(uc2) == 1 and uc2 not in products_off                  # one linear64 on the canonical representatives
    assert len(products_on) == len(products_off)
    # one walk, all the table layers in it, behind the representatives' launch; no rows written
    assert walks_on == [(None, 9 if pool_tables else 6)] and walks_off == [(None, 6 if pool_tables else 3)]
    assert _renamed(names_on, names_off, layers), (names_on, names_off)


@pytest.mark.parametrize("name", ["golden", "one neighborhood", "mutag24 class bound", "mutag24 row bound", "two layers"])
def test_ineligible_batch_launches_the_parents_kernels(models, name):
    if name == "two layers":
        from_model = _model(2)
        batch = _batch(synthetic.mutag_shaped(24))
    else:
        from_model = models[8]
        batch = {"golden": lambda: _batch(golden_graphs()), "one neighborhood": lambda: _batch([_path(2)], lowered=False),
                 "mutag24 class bound": lambda: _batch(synthetic.mutag_shaped(24)),
                 "mutag24 row bound": lambda: _batch(synthetic.mutag_shaped(24))}[name]()
    if name == "mutag24 class bound":
        batch.LAYER3_MIN_ROWS_PER_CLASS = NeighborhoodBatch.LAYER3_MIN_ROWS_PER_CLASS
    if name == "mutag24 row bound":
        batch.LAYER3_MIN_ROWS = NeighborhoodBatch.LAYER3_MIN_ROWS
    if name != "two layers":
        assert batch.layer3_table_index() is None
    from_model.graph_to_count(batch)
    on, names_on, layers_on, products_on, walks_on = _pass(from_model, batch, True)
    off, names_off, layers_off, products_off, walks_off = _pass(from_model, batch, False)
    assert names_on == names_off and layers_on == layers_off and products_on == products_off
    assert [w[1] for w in walks_on] == [w[1] for w in walks_off]
    assert torch.isfinite(on).all() and torch.equal(on, off)


def test_a_block_at_the_default_bounds_takes_the_path(models):
    """nothing lowered: the 24-graph set x188 has 525 460 count rows (>= 2^19) in 1 563 classes; x94 (262 730 rows) keeps
    the parent's launches"""
    nm = models[8]
    batch = _batch(synthetic.mutag_shaped(24).replicate(188), lowered=False)
    assert batch.num_count >= NeighborhoodBatch.LAYER3_MIN_ROWS == batch.LAYER3_MIN_ROWS >= 1 << 19
    tab3 = batch.layer3_table_index()
    assert tab3 is not None
    u2, u3 = (batch.layer2_table_index()[1].numel() - 1) // 4, tab3[3].numel()
    assert (u2, u3) == (360, 1563)           # (the unsorted partition's classes; replication adds none)
    nm.graph_to_count(batch)
    on, names_on, layers_on, _, walks_on = _pass(nm, batch, True)
    off, names_off, _, _, walks_off = _pass(nm, batch, False)
    assert torch.isfinite(on).all() and torch.equal(on, off)
    assert walks_on == [(None, 9)] and walks_off == [(None, 6)] and _renamed(names_on, names_off, 8)
    assert [c for c in layers_on if c[1] == u3] == [(u2, u3, u3, True)]
    batch = _batch(synthetic.mutag_shaped(24).replicate(94), lowered=False)
    assert batch.num_count == 262730 and batch.layer3_table_index() is None
    nm.graph_to_count(batch)
    on, names_on, *_ = _pass(nm, batch, True)
    off, names_off, *_ = _pass(nm, batch, False)
    assert names_on == names_off and torch.equal(on, off)


KEYS = ("neigh_count", "node_count", "graph_neigh_count", "graph_gossip_count")


def test_pipeline_outputs_are_equal_and_a_captured_replay_equals_the_eager_pass():
    from desco_amd.pipeline import InferencePipeline
    nm, gm = make_models(seed=0)
    nm, gm = nm.to(DEV), gm.to(DEV)
    nm.set_queries(standard_queries()[0])
    pipe = InferencePipeline(nm, gm, synthetic.mutag_shaped(188), depth=4, device=DEV)
    for b in pipe.neigh_batches:
        _lower(b)
    assert all(b.layer3_table_index() is not None for b in pipe.neigh_batches)
    pipe.run()                               # (the first pass of a model also folds and splits its weights)
    old = GM.THIRD_LAYER_TABLE
    res = {}
    try:
        for on in (True, False):
            GM.THIRD_LAYER_TABLE = on
            ops.PROFILER.reset()
            ops.PROFILER.enabled = True
            res[on] = {k: v.clone() for k, v in pipe.run().items() if k in KEYS}
            torch.cuda.synchronize()
            res[on]["selfidx"] = [r[0] for r in ops.PROFILER.records].count(SELFIDX)
            ops.PROFILER.enabled = False
        GM.THIRD_LAYER_TABLE = True
        pipe.capture()
        rep = pipe.run_graph()
        torch.cuda.synchronize()
    finally:
        GM.THIRD_LAYER_TABLE = old
        ops.PROFILER.enabled = False
        ops.PROFILER.reset()
    assert res[True]["selfidx"] == 2 * len(pipe.neigh_batches) and res[False]["selfidx"] == len(pipe.neigh_batches)
    for k in KEYS:
        assert torch.isfinite(res[True][k]).all() and torch.equal(res[True][k], res[False][k]), k
        assert torch.equal(res[True][k], rep[k]), k
