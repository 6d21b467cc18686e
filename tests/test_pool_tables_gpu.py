"""gnn_model.POOL_TABLES: the pooled partial sums of the two table layers of a molecule batch -- X_1 = table1[row_id], X_2 =
table2[cls] -- from ONE walk over the count rows (desco_table_rows_pool2_f32, tables staged in LDS where they fit) instead
of the two launches desco_degree_affine_pool_f32 (on the CSR) and desco_table_rows_pool_f32 (on the table).  Everything here
is a bit-for-bit comparison (torch.equal) against those two launches with the same pooling index: the rows are the same rows
and the running sums the same sums in the same order.  Outputs are pre-filled with NaN.

The pass takes the merged launch on blocks of at least NeighborhoodBatch.POOL_TABLES_MIN_ROWS count rows (a bound on the
profit); the small blocks here lower it on their own batch object, with the other LAYER2_* bounds, so that the path is taken."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import desco_amd.gnn_model as GM  # noqa: E402
from desco_amd import _lib, ops, synthetic  # noqa: E402
from desco_amd.batch import NeighborhoodBatch  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402
from desco_amd.partition import build_partition  # noqa: E402

import pool_reference as P  # noqa: E402
from helpers import golden_graphs, make_models, neigh_args, standard_queries  # noqa: E402

DEV = "cuda"
NAN = float("nan")
S = 4


def _cap():
    """table rows that fit in the kernel's LDS budget"""
    return _lib.lib().desco_table_rows_pool2_lds_bytes() // 256


# ---- (a) the merged launch against the two launches it replaces -------------------------------------------------------------
def _case(seg_lens, U1, U2, seed, num_rows=None):
    """N = sum(seg_lens) rows in pooling segments of ``seg_lens`` rows.  First layer: U1 distinct degree tuples (their
    row-pointer array, the table the closed-form layer makes of it), every row's tuple id and the rows' full CSR row
    pointers; second layer: a random table [U2, 64] and every row's class.  The LAST id of either table belongs to the last
    row (so that the table's last row is read).  ``num_rows``: the launches run on that prefix of the rows (the pooling
    index stays the whole layout's: the prefix's last segment is then left open at its end)."""
    g = torch.Generator().manual_seed(seed)
    sp = P.seg_ptr_of(np.asarray(seg_lens, dtype=np.int64))
    N = int(sp[-1])
    n = N if num_rows is None else num_rows
    deg = torch.randint(0, 5, (U1, S), generator=g)
    deg[::7] = 0
    ids1 = torch.randint(0, max(U1 - 1, 1), (N,), generator=g)
    ids2 = torch.randint(0, max(U2 - 1, 1), (N,), generator=g)
    ids1[n - 1], ids2[n - 1] = U1 - 1, U2 - 1
    _, ns, (bits, slot) = P.slots_of(sp, N)
    i32 = lambda a: torch.as_tensor(a, dtype=torch.int32).reshape(-1).contiguous().to(DEV)    # noqa: E731
    uptr = i32(torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(deg.reshape(-1), 0)]))
    coef = (torch.randn(S + 1, 64, generator=g) / 4).to(DEV)
    table1 = torch.full((U1, 64), NAN, device=DEV)
    ops.degree_affine(uptr, 0, U1, S, coef, ops.ACT_RELU, 0.0, table1)
    return dict(N=N, n=n, ns=ns, U1=U1, U2=U2, deg=deg, coef=coef, table1=table1, ids1=i32(ids1), ids2=i32(ids2),
                table2=torch.randn(U2, 64, generator=g).to(DEV),
                bits=torch.from_numpy(bits.view(np.int32)).to(DEV), slot=torch.from_numpy(slot).to(DEV))


def _reference(c, ids1=None, ids2=None):
    """(part1, out2, part2) of the two existing launches: degree_affine_pool on the rows' CSR, table_rows_pool on table2"""
    ids1 = c["ids1"] if ids1 is None else ids1
    ids2 = c["ids2"] if ids2 is None else ids2
    n, ns = c["n"], c["ns"]
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(c["deg"][ids1.cpu().long()].reshape(-1), 0)])
    part1 = torch.full((ns + 1, 64), NAN, device=DEV)
    ops.degree_affine_pool(ptr.to(torch.int32).to(DEV), n, S, c["coef"], ops.ACT_RELU, 0.0, None, (c["bits"], c["slot"], part1))
    out2 = torch.full((c["N"] + 1, 64), NAN, device=DEV)
    part2 = torch.full((ns + 1, 64), NAN, device=DEV)
    ops.table_rows_pool(c["table2"], ids2, n, out2, (c["bits"], c["slot"], part2))
    return part1, out2, part2


def _same(a, b):
    """bit-equal where b is a number, NaN (untouched) where b is NaN"""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def _merged(c, store, ids1=None, ids2=None, table1=None, table2=None, out=None):
    ids1 = c["ids1"] if ids1 is None else ids1
    ids2 = c["ids2"] if ids2 is None else ids2
    part1 = torch.full((c["ns"] + 1, 64), NAN, device=DEV)
    part2 = torch.full((c["ns"] + 1, 64), NAN, device=DEV)
    if out is None and store:
        out = torch.full((c["N"] + 1, 64), NAN, device=DEV)
    ops.table_rows_pool(c["table2"] if table2 is None else table2, ids2, c["n"], out,
                        (c["bits"], c["slot"], part2, c["table1"] if table1 is None else table1, ids1, part1))
    return part1, out, part2


def _check(c):
    ref1, ref_out, ref2 = _reference(c)
    # (the references wrote every slot of the rows they were given and nothing else -- what _same then asks of the merged launch)
    used = int(torch.isfinite(ref2[:, 0]).sum())
    assert 0 < used <= c["ns"] and torch.isfinite(ref1[:used]).all() and torch.isnan(ref1[used:]).all()
    assert torch.isfinite(ref_out[:c["n"]]).all() and torch.isnan(ref_out[c["n"]:]).all()
    part1, out, part2 = _merged(c, True)
    assert _same(part1, ref1) and _same(part2, ref2) and _same(out, ref_out)
    part1, out, part2 = _merged(c, False)                                  # out = None: the partials alone
    assert out is None and _same(part1, ref1) and _same(part2, ref2)
    return ref1, ref_out, ref2


_SWEEP = [int(v) for v in P.layout("sweep33")]                # segments of 1 .. 33 rows, each at every tile alignment
# one row .. two tiles and one row .. five tiles and one row, one segment each; the sweep (with it segments that span three
# tiles).  The grid is persistent (one block of 16 waves per CU, 256 blocks at most) and a wave requests the index of four
# tiles at once, 4 096 tiles apart: 72 000 rows are 4 500 tiles, so that some waves have a second tile in their group and most
# do not; 264 000 rows are 16 500 tiles, more than 4 x 4 096: some waves walk on to a second group, whose index was
# requested during the first
CASES = [(f"n{n} u{u}", [n], u, u, None) for n in (1, 15, 16, 17, 33, 16 * 5 + 1) for u in (1, 2, 300)] + \
        [("sweep33 u300 u250", _SWEEP, 300, 250, None), ("sweep33 head u2 u1", _SWEEP[:160], 2, 1, None),
         ("ones u1 u300", [1] * 100, 1, 300, None), ("1..33 u300", list(range(1, 34)) + list(range(33, 0, -1)), 300, 300, None),
         ("open last segment", [5, 33, 20, 7], 300, 300, 5 + 33 + 9), ("open last segment at a tile end", [30, 30], 2, 300, 48),
         ("a second tile per wave", [24] * 3000, 300, 300, None), ("a second group per wave", [24] * 11000, 300, 300, None)]


@pytest.mark.parametrize("name,seg_lens,U1,U2,n", CASES, ids=[c[0] for c in CASES])
def test_merged_launch_leaves_what_the_two_launches_leave(name, seg_lens, U1, U2, n):
    assert U1 + U2 <= _cap()                                              # (both tables in LDS)
    _check(_case(seg_lens, U1, U2, 300 + len(seg_lens) + U1 + U2, n))


def _budget_cases():
    cap = 624           # (asserted equal to the library's in the test: the ids of the parametrisation are built without it)
    return [("table2 above the budget", 300, cap + 1), ("table1 above the budget", cap + 1, 300),
            ("both above the budget", cap + 1, cap + 2), ("each fits, not both: table1 larger", 400, 300),
            ("each fits, not both: table2 larger", 300, 400), ("both fill the budget", cap - 300, 300),
            ("table1 fills the budget", cap, 1)]


@pytest.mark.parametrize("name,U1,U2", _budget_cases(), ids=[c[0] for c in _budget_cases()])
def test_tables_beyond_the_lds_budget_are_read_from_global_memory(name, U1, U2):
    """the four forms of the kernel (a table in LDS or in global memory, per table) leave the same bits"""
    assert _cap() == 624
    _check(_case(_SWEEP[:200] + [33, 1, 16], U1, U2, 500 + U1 + U2))


def test_strided_tables_and_a_column_block_of_a_wider_output():
    c = _case(_SWEEP[:120], 300, 250, 77)
    ref1, ref_out, ref2 = _reference(c)
    wide1 = torch.full((300, 128), NAN, device=DEV)
    wide1[:, 64:] = c["table1"]
    wide2 = torch.full((250, 192), NAN, device=DEV)
    wide2[:, :64] = c["table2"]
    out = torch.full((c["N"], 192), NAN, device=DEV)
    part1, _, part2 = _merged(c, True, table1=wide1[:, 64:], table2=wide2[:, :64], out=out[:, 64:128])
    assert _same(part1, ref1) and _same(part2, ref2) and torch.equal(out[:, 64:128], ref_out[:c["N"]])
    assert torch.isnan(out[:, :64]).all() and torch.isnan(out[:, 128:]).all()


@pytest.mark.parametrize("U1,U2", [(300, 250), (625, 700)], ids=["lds", "global"])
def test_ids_outside_their_table_are_clamped(U1, U2):
    """an id outside its table is the caller's error (desco_index_range_check_i32 finds it): the kernel reads the nearest
    table row and writes nothing out of bounds"""
    c = _case(_SWEEP[:60], U1, U2, 91)
    ids1, ids2 = c["ids1"].clone(), c["ids2"].clone()
    ids1[3], ids1[40], ids2[17], ids2[41] = U1 + 5, -2, -(2 ** 31), 2 ** 31 - 1
    ref1, ref_out, ref2 = _reference(c, ids1.clamp(0, U1 - 1), ids2.clamp(0, U2 - 1))
    part1, out, part2 = _merged(c, True, ids1=ids1, ids2=ids2)
    assert _same(part1, ref1) and _same(part2, ref2) and _same(out, ref_out)


def test_argument_errors_are_einval():
    L = _lib.lib()
    c = _case([5, 12], 3, 4, 1)
    out = torch.full((17, 64), NAN, device=DEV)
    part1 = torch.full((c["ns"], 64), NAN, device=DEV)
    part2 = torch.full((c["ns"], 64), NAN, device=DEV)
    p = lambda t: t.data_ptr()    # noqa: E731
    good = dict(t1=p(c["table1"]), ld1=64, n1=3, ids1=p(c["ids1"]), part1=p(part1), t2=p(c["table2"]), ld2=64, n2=4,
                ids2=p(c["ids2"]), part2=p(part2), n=17, out=p(out), ldo=64, bits=p(c["bits"]), slot=p(c["slot"]))

    def call(**kw):
        a = dict(good, **kw)
        return L.desco_table_rows_pool2_f32(*[a[k] for k in good], None)

    for kw in (dict(t1=None), dict(t2=None), dict(ids1=None), dict(ids2=None), dict(part1=None), dict(part2=None),
               dict(bits=None), dict(slot=None), dict(n=-1), dict(n1=0), dict(n2=0), dict(n1=2 ** 31), dict(ld1=32), dict(ld2=66),
               dict(t1=good["t1"] + 4), dict(t2=good["t2"] + 4), dict(part1=good["part1"] + 4), dict(part2=good["part2"] + 4),
               dict(part2=good["part1"]), dict(out=good["out"] + 4), dict(ldo=66), dict(ldo=32), dict(out=good["t1"]),
               dict(out=good["t2"])):
        assert call(**kw) == -1, kw
        assert b"desco_table_rows_pool2_f32" in L.desco_last_error(), (kw, L.desco_last_error())
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(part1).all() and torch.isnan(part2).all()      # refused before any launch
    assert call(n=0) == 0                                                                          # nothing to do
    assert call() == 0
    torch.cuda.synchronize()
    ref1, ref_out, ref2 = _reference(c)
    assert torch.equal(out, ref_out[:17]) and torch.equal(part1, ref1[:c["ns"]]) and torch.equal(part2, ref2[:c["ns"]])


# ---- (b) the pass: switch on against switch off -------------------------------------------------------------------------------
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
    return {L: _model(L) for L in (8, 3, 2)}


def _lower(b):
    b.LAYER2_MIN_ROWS_PER_CLASS = 1
    b.LAYER2_GATHER_MIN_ROWS = 0
    b.POOL_TABLES_MIN_ROWS = 0
    return b


def _batch(graphs, lowered=True):
    gs = graphs if isinstance(graphs, GraphSet) else GraphSet.from_edge_lists(graphs)
    b = NeighborhoodBatch(build_partition(gs, 4), DEV)
    return _lower(b) if lowered else b


def _pass(nm, batch, on, gather=True):
    """(logits, per table_rows_pool call (out, entries of ``pool``), kernel names) of one inference pass"""
    calls = []
    real_rows = ops.table_rows_pool

    def spy_rows(table, cls, n, out, pool):
        calls.append((out, len(pool)))
        real_rows(table, cls, n, out, pool)

    old = GM.POOL_TABLES, GM.SECOND_LAYER_GATHER
    GM.POOL_TABLES, GM.SECOND_LAYER_GATHER, ops.table_rows_pool = on, gather, spy_rows
    ops.PROFILER.reset()
    ops.PROFILER.enabled = True
    try:
        out = nm.graph_to_count(batch).clone()
        torch.cuda.synchronize()
        names = [r[0] for r in ops.PROFILER.records]
    finally:
        (GM.POOL_TABLES, GM.SECOND_LAYER_GATHER), ops.table_rows_pool = old, real_rows
        ops.PROFILER.enabled = False
        ops.PROFILER.reset()
    return out, calls, names


def _one_launch_less(names_on, names_off):
    """the same launches in the same order but the first layer's pooled launch on the count rows"""
    missing = [k for k in range(len(names_off)) if names_off[:k] + names_off[k + 1:] == names_on]
    return len(names_on) == len(names_off) - 1 and bool(missing) and names_off[missing[0]] == "degree_affine_kernel"


ELIGIBLE = {"mutag24": lambda: _batch(synthetic.mutag_shaped(24)), "small": lambda: _batch(SMALL)}


@pytest.mark.parametrize("layers,gather", [(8, True), (8, False), (3, True), (2, True)],
                         ids=["L8", "L8 X_2 stored", "L3", "L2"])
@pytest.mark.parametrize("name", list(ELIGIBLE))
def test_eligible_batch_takes_the_merged_launch_and_changes_no_bit(models, name, layers, gather):
    nm, batch = models[layers], ELIGIBLE[name]()
    assert batch.layer2_table_index() is not None
    nm.graph_to_count(batch)                 # (the first pass of a model also folds and splits its weights)
    on, calls_on, names_on = _pass(nm, batch, True, gather)
    off, calls_off, names_off = _pass(nm, batch, False, gather)
    assert torch.isfinite(on).all() and torch.equal(on, off)
    stored = layers > 2 and not gather                                    # (X_2's count rows: written by the same launch)
    assert len(calls_on) == 1 and calls_on[0][1] == 6 and (calls_on[0][0] is not None) == stored
    assert len(calls_off) == 1 and calls_off[0][1] == 3 and (calls_off[0][0] is not None) == stored
    assert _one_launch_less(names_on, names_off), (names_on, names_off)
    assert names_on.count("table_rows_pool_kernel") == names_off.count("table_rows_pool_kernel") == 1


def test_a_block_at_the_default_bounds_takes_the_merged_launch(models):
    """nothing lowered: the 24-graph set x94 has 262 730 count rows (>= 2^18) in 360 classes"""
    nm = models[8]
    batch = _batch(synthetic.mutag_shaped(24).replicate(94), lowered=False)
    assert batch.num_count >= NeighborhoodBatch.POOL_TABLES_MIN_ROWS == batch.POOL_TABLES_MIN_ROWS == 1 << 18
    assert batch.layer2_table_index() is not None
    nm.graph_to_count(batch)
    on, calls_on, names_on = _pass(nm, batch, True)
    off, calls_off, names_off = _pass(nm, batch, False)
    assert torch.isfinite(on).all() and torch.equal(on, off)
    assert calls_on == [(None, 6)] and calls_off == [(None, 3)] and _one_launch_less(names_on, names_off)


def test_a_block_below_the_row_bound_keeps_the_two_launches(models):
    nm = models[8]
    for bound, taken in ((None, False), ("nc", True), ("nc + 1", False)):
        batch = _batch(synthetic.mutag_shaped(24))
        batch.POOL_TABLES_MIN_ROWS = (NeighborhoodBatch.POOL_TABLES_MIN_ROWS if bound is None else
                                      batch.num_count + (bound == "nc + 1"))
        assert batch.num_count < NeighborhoodBatch.POOL_TABLES_MIN_ROWS
        nm.graph_to_count(batch)
        on, calls_on, names_on = _pass(nm, batch, True)
        off, _, names_off = _pass(nm, batch, False)
        assert torch.equal(on, off) and (calls_on == [(None, 6)]) == taken
        assert _one_launch_less(names_on, names_off) if taken else names_on == names_off


@pytest.mark.parametrize("name", ["golden", "one neighborhood", "mutag24 class bound"])
def test_ineligible_batch_launches_the_same_kernels(models, name):
    """no second-layer table: today's launches, kernel for kernel (the row bound lowered, so that it is not what refuses)"""
    batch = {"golden": lambda: _batch(golden_graphs(), lowered=False), "one neighborhood": lambda: _batch([_path(2)], lowered=False),
             "mutag24 class bound": lambda: _batch(synthetic.mutag_shaped(24), lowered=False)}[name]()
    batch.POOL_TABLES_MIN_ROWS = 0
    assert batch.layer2_table_index() is None
    nm = models[8]
    nm.graph_to_count(batch)
    on, calls_on, names_on = _pass(nm, batch, True)
    off, calls_off, names_off = _pass(nm, batch, False)
    assert names_on == names_off and "table_rows_pool_kernel" not in names_on and not calls_on and not calls_off
    assert torch.isfinite(on).all() and torch.equal(on, off)


# ---- (c) the pipeline, eager and captured -------------------------------------------------------------------------------------
KEYS = ("neigh_count", "node_count", "graph_neigh_count", "graph_gossip_count")


def test_pipeline_outputs_are_equal_and_a_captured_replay_equals_the_eager_pass():
    from desco_amd.pipeline import InferencePipeline
    nm, gm = make_models(seed=0)
    nm, gm = nm.to(DEV), gm.to(DEV)
    nm.set_queries(standard_queries()[0])
    pipe = InferencePipeline(nm, gm, synthetic.mutag_shaped(24), depth=4, device=DEV)
    for b in pipe.neigh_batches:
        _lower(b)
    assert all(b.layer2_table_index() is not None for b in pipe.neigh_batches)
    pipe.run()                               # (the first pass of a model also folds and splits its weights)
    old = GM.POOL_TABLES
    res = {}
    try:
        for on in (True, False):
            GM.POOL_TABLES = on
            ops.PROFILER.reset()
            ops.PROFILER.enabled = True
            res[on] = {k: v.clone() for k, v in pipe.run().items() if k in KEYS}
            torch.cuda.synchronize()
            res[on]["first"] = [r[0] for r in ops.PROFILER.records].count("degree_affine_kernel")
            ops.PROFILER.enabled = False
        GM.POOL_TABLES = True
        pipe.capture()
        rep = pipe.run_graph()
        torch.cuda.synchronize()
    finally:
        GM.POOL_TABLES = old
        ops.PROFILER.enabled = False
        ops.PROFILER.reset()
    assert res[True]["first"] == res[False]["first"] - len(pipe.neigh_batches)
    for k in KEYS:
        assert torch.isfinite(res[True][k]).all() and torch.equal(res[True][k], res[False][k]), k
        assert torch.equal(res[True][k], rep[k]), k
