"""gnn_model.DEEP_LAYER_TABLES: the SHMP layers beyond the third on one representative per class of their output
(NeighborhoodBatch.deep_table_index, levels 4 .. K), X_4 .. X_K's count rows never written, layer K + 1 gathering from table K,
the partial sums of all table layers from the walk behind the last representatives' launch.  Everything is a bit-for-bit
comparison (torch.equal) of the pass with the switch on against the pass with the switch off: the layer kernel's arithmetic is
row-local and, with at most 8 sources per row, its gather order a function of the row alone.

The pass takes the path on blocks of at least NeighborhoodBatch.DEEP_TABLE_MIN_ROWS count rows (a bound on the profit); the
small blocks here lower it and the other profit bounds on their own batch object, and set the depth they test."""
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
    return {L: _model(L) for L in (8, 5, 4)}


def _lower(b, max_level=8):
    b.LAYER2_MIN_ROWS_PER_CLASS = b.LAYER3_MIN_ROWS_PER_CLASS = b.DEEP_TABLE_MIN_ROWS_PER_CLASS = 1
    b.LAYER2_GATHER_MIN_ROWS = b.LAYER3_MIN_ROWS = b.POOL_TABLES_MIN_ROWS = b.DEEP_TABLE_MIN_ROWS = 0
    b.DEEP_TABLE_MAX_LEVEL = max_level
    return b


def _batch(graphs, lowered=True, max_level=8):
    gs = graphs if isinstance(graphs, GraphSet) else GraphSet.from_edge_lists(graphs)
    b = NeighborhoodBatch(build_partition(gs, 4), DEV)
    return _lower(b, max_level) if lowered else b


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

    old = GM.DEEP_LAYER_TABLES
    GM.DEEP_LAYER_TABLES = on
    ops.shmp_layer, ops.linear64, ops.table_rows_pool = spy_layer, spy_linear, spy_walk
    ops.PROFILER.reset()
    ops.PROFILER.enabled = True
    try:
        out = nm.graph_to_count(batch).clone()
        torch.cuda.synchronize()
        names = [r[0] for r in ops.PROFILER.records]
    finally:
        GM.DEEP_LAYER_TABLES = old
        ops.shmp_layer, ops.linear64, ops.table_rows_pool = real
        ops.PROFILER.enabled = False
        ops.PROFILER.reset()
    return out, names, layers, products, walks


GRAPHS = {"mutag24": lambda: synthetic.mutag_shaped(24), "small": lambda: SMALL, "cox2 cut": lambda: synthetic.cox2_shaped(12)}
# (layers of the model, depth bound on the batch): K = L = 8; K = 6 < L; K = L = 5 under a deeper bound; the only new level is the
# model's last layer
DEPTHS = [(8, 8), (8, 6), (5, 8), (4, 8)]


@pytest.mark.parametrize("layers,max_level", DEPTHS, ids=[f"L{a} depth bound {b}" for a, b in DEPTHS])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_eligible_batch_takes_the_path_and_changes_no_bit(models, name, layers, max_level):
    nm, batch = models[layers], _batch(GRAPHS[name](), max_level=max_level)
    assert batch.num_count < 6000
    K = min(layers, max_level)
    tab3, deep = batch.layer3_table_index(), batch.deep_table_index()
    assert tab3 is not None and len(deep) == max_level - 3
    nc, n = batch.num_count, batch.num_rows
    u = {2: (batch.layer2_table_index()[1].numel() - 1) // 4, 3: tab3[3].numel()}
    u.update({k: lv[3].numel() for k, lv in enumerate(deep, 4)})
    uc = {k: lv[6].numel() for k, lv in enumerate(deep, 4)}
    assert not {nc, n, n - nc} & set(u.values())                       # (so that a launch on representatives is known by its rows)
    nm.graph_to_count(batch)                 # (the first pass of a model also folds and splits its weights)
    on, names_on, layers_on, products_on, walks_on = _pass(nm, batch, True)
    off, names_off, layers_off, products_off, walks_off = _pass(nm, batch, False)
    assert torch.isfinite(on).all() and torch.equal(on, off)
    # one count launch on U_k rows per table level, in order: sources and own rows in the table before, the output table k
    assert [c for c in layers_on if c[3] and c[1] != nc] == [(u[k - 1], u[k], u[k], True) for k in range(3, K + 1)]
    assert [c for c in layers_off if c[3] and c[1] != nc] == [(u[2], u[3], u[3], True)]
    # no [N, 64] output for the layers 4 .. K (the parent's last count launch stores no rows either)
    assert sum(c[2] == n for c in layers_off) - sum(c[2] == n for c in layers_on) == K - 3 - (K == layers)
    # layer K + 1, if the model has one, gathers from table K, the count launch with its own rows through the classes; the
    # canonical launches of the layers 5 .. K + 1 gather from tables as well
    assert [c for c in layers_on if c[1] == nc and c[3]] == ([(u[K], nc, None if layers == K + 1 else n, True)] if layers > K else [])
    assert [c for c in layers_off if c[1] == nc and c[3]] == [(u[3], nc, None if layers == 4 else n, True)]
    canon_x = lambda ls: sum(c[1] == n - nc and c[0] == n for c in ls)    # noqa: E731  (canonical launches that read an [N, 64] X)
    assert canon_x(layers_off) - canon_x(layers_on) == min(K, layers - 1) - 3
    assert names_on.count(SELFIDX) == K - 2 + (layers > K) and names_off.count(SELFIDX) == 2
    # the linear64 launches of the table levels run on the canonical representatives
    assert len(products_on) == len(products_off)
    assert Counter(products_on) - Counter(products_off) == Counter(uc[k] for k in range(4, K + 1))
    assert (Counter(products_off) - Counter(products_on)).keys() <= {n - nc}
    # one call for the partial sums of the K table layers, behind the last representatives' launch; no rows written
    assert walks_on == [(None, 3 * K)] and walks_off == [(None, 9)]
    assert names_on.count(WALK) == (1 if K <= ops.POOL_WALK_LAYERS else 2) and names_off.count(WALK) == 1
    assert len(names_on) - names_on.count(WALK) == len(names_off) - 1   # (as many of the project's launches besides)


@pytest.mark.parametrize("name", ["row bound", "rows per class", "class bound", "depth bound 3", "three layers"])
def test_ineligible_batch_launches_the_parents_kernels(models, name):
    nm = _model(3) if name == "three layers" else models[8]
    batch = _batch(synthetic.mutag_shaped(24))
    if name == "row bound":
        batch.DEEP_TABLE_MIN_ROWS = NeighborhoodBatch.DEEP_TABLE_MIN_ROWS
    elif name == "rows per class":
        batch.DEEP_TABLE_MIN_ROWS_PER_CLASS = batch.num_count
    elif name == "class bound":
        batch.DEEP_TABLE_MAX_CLASSES = 8
    elif name == "depth bound 3":
        batch.DEEP_TABLE_MAX_LEVEL = 3
    assert batch.layer3_table_index() is not None
    if name != "three layers":
        assert batch.deep_table_index() == []
    nm.graph_to_count(batch)
    on, names_on, layers_on, products_on, walks_on = _pass(nm, batch, True)
    off, names_off, layers_off, products_off, walks_off = _pass(nm, batch, False)
    assert names_on == names_off and layers_on == layers_off and products_on == products_off
    assert [w[1] for w in walks_on] == [w[1] for w in walks_off] == [9]
    assert torch.isfinite(on).all() and torch.equal(on, off)


def test_the_default_row_bound(models):
    """nothing lowered: a block just under DEEP_TABLE_MIN_ROWS count rows launches the parent's kernels, the next larger one
    takes the path"""
    nm = models[8]
    rows = 2795                                                        # count rows of the 24-graph set
    bound = NeighborhoodBatch.DEEP_TABLE_MIN_ROWS
    assert bound >= 1 << 20
    under = _batch(synthetic.mutag_shaped(24).replicate((bound - 1) // rows), lowered=False)
    assert bound - rows <= under.num_count < bound == under.DEEP_TABLE_MIN_ROWS
    assert under.layer3_table_index() is not None and under.deep_table_index() == []
    nm.graph_to_count(under)
    on, names_on, layers_on, products_on, walks_on = _pass(nm, under, True)
    off, names_off, layers_off, products_off, walks_off = _pass(nm, under, False)
    assert names_on == names_off and layers_on == layers_off and products_on == products_off and walks_on == walks_off
    assert torch.isfinite(on).all() and torch.equal(on, off)
    del under
    over = _batch(synthetic.mutag_shaped(24).replicate((bound - 1) // rows + 1), lowered=False)
    assert over.num_count >= bound
    deep = over.deep_table_index()
    assert len(deep) == NeighborhoodBatch.DEEP_TABLE_MAX_LEVEL - 3
    nm.graph_to_count(over)
    on, names_on, layers_on, _, walks_on = _pass(nm, over, True)
    off, names_off, *_ = _pass(nm, over, False)
    assert torch.isfinite(on).all() and torch.equal(on, off)
    if deep:
        assert walks_on == [(None, 3 * (3 + len(deep)))] and [c[1] for c in layers_on if c[3] and c[1] != over.num_count][1:] == \
            [lv[3].numel() for lv in deep]
    else:
        assert names_on == names_off


KEYS = ("neigh_count", "node_count", "graph_neigh_count", "graph_gossip_count")


def test_pipeline_outputs_are_equal_and_a_captured_replay_equals_the_eager_pass():
    from desco_amd.pipeline import InferencePipeline
    nm, gm = make_models(seed=0)
    nm, gm = nm.to(DEV), gm.to(DEV)
    nm.set_queries(standard_queries()[0])
    pipe = InferencePipeline(nm, gm, synthetic.mutag_shaped(188), depth=4, device=DEV)
    for b in pipe.neigh_batches:
        _lower(b)
    assert all(len(b.deep_table_index()) == 5 for b in pipe.neigh_batches)
    pipe.run()                               # (the first pass of a model also folds and splits its weights)
    old = GM.DEEP_LAYER_TABLES
    res = {}
    try:
        for on in (True, False):
            GM.DEEP_LAYER_TABLES = on
            ops.PROFILER.reset()
            ops.PROFILER.enabled = True
            res[on] = {k: v.clone() for k, v in pipe.run().items() if k in KEYS}
            torch.cuda.synchronize()
            res[on]["selfidx"] = [r[0] for r in ops.PROFILER.records].count(SELFIDX)
            ops.PROFILER.enabled = False
        GM.DEEP_LAYER_TABLES = True
        pipe.capture()
        rep = pipe.run_graph()
        torch.cuda.synchronize()
    finally:
        GM.DEEP_LAYER_TABLES = old
        ops.PROFILER.enabled = False
        ops.PROFILER.reset()
    assert res[True]["selfidx"] == 6 * len(pipe.neigh_batches) and res[False]["selfidx"] == 2 * len(pipe.neigh_batches)
    for k in KEYS:
        assert torch.isfinite(res[True][k]).all() and torch.equal(res[True][k], res[False][k]), k
        assert torch.equal(res[True][k], rep[k]), k
