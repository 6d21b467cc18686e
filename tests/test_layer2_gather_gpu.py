"""gnn_model.SECOND_LAYER_GATHER: the third layer's launches gather from the table of the second layer's distinct count rows
(desco_shmp_layer_selfidx_f16x3_f32: sources AND own rows addressed through the rows' classes), X_2's count rows are never
written.  Everything here is a bit-for-bit comparison (torch.equal): the SELFIDX instantiation changes where a row is read,
not what is computed with it.  Outputs are pre-filled with NaN.

The index refuses a block with fewer than 8 rows per class and the pass keeps X_2 for blocks of fewer than 2^18 count rows
(bounds on the profit); the small blocks here lower both on their own batch object so that the path is taken."""
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
PLAIN = "shmp_layer16_kernel<3,2,f16x3>"
SELFIDX = "shmp_layer16_kernel<3,2,f16x3,selfidx>"


def _path(n):
    return (n, [(i, i + 1) for i in range(n - 1)])


def _ring(n):
    return (n, [(i, (i + 1) % n) for i in range(n)])


def _star(k):
    return (k + 1, [(0, v) for v in range(1, k + 1)])


SMALL = ([_path(n) for n in range(2, 8)] + [_ring(5), _ring(6)] + [_star(k) for k in range(1, 5)]) * 3


# ---- (a) the SELFIDX launch on the table against the pooled narrow launch on the materialised rows ---------------------------
def _case(seg_lens, U, seed, heavy_row=None, dense_tile=None):
    """N = sum(seg_lens) rows in pooling segments of ``seg_lens`` rows, a table T [U, 64] and the rows' classes (the LAST class
    belongs to the last row alone), a 4-slot CSR: slots 0 and 1 hold row ids, slot 2 (table slot 0) is empty, slot 3 at most one
    row of ytab [11, 64] (global id N + t, ytab_row0 = N).  ``heavy_row``: that row gets 25 slot-0 sources (more than the 20 of
    the batched steps: the cooperative path); ``dense_tile``: the 16 rows of that tile get 7 + 7 sources each (224 ids: more
    than the 200 staged per tile, the rest read from global memory)."""
    rng = np.random.default_rng(seed)
    S, n_tab = 4, 11
    sp = P.seg_ptr_of(np.asarray(seg_lens, dtype=np.int64))
    N = int(sp[-1])
    deg = rng.integers(0, 4, (N, S))
    deg[:, 2] = 0
    deg[:, 3] = rng.integers(0, 2, N)
    deg[::5] = 0                                                          # rows without any source
    deg[1::5, :2] = 0                                                     # ... and with a table source alone
    if heavy_row is not None:
        deg[heavy_row, 0] = 25
    if dense_tile is not None:
        deg[16 * dense_tile:16 * dense_tile + 16, :2] = 7
    ptr = np.concatenate([[0], np.cumsum(deg.reshape(-1))])
    slot_of = np.repeat(np.tile(np.arange(S), N), deg.reshape(-1))
    col = np.where(slot_of < 2, rng.integers(0, N, slot_of.size), N + rng.integers(0, n_tab, slot_of.size))
    cls = rng.integers(0, max(U - 1, 1), N)
    cls[N - 1] = U - 1
    col_cls = np.where(slot_of < 2, cls[np.minimum(col, N - 1)], col)     # slot-0/1 sources through the classes
    _, ns, (bits, slot) = P.slots_of(sp, N)
    g = torch.Generator().manual_seed(seed)
    i32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32).reshape(-1).to(DEV)    # noqa: E731
    return dict(N=N, U=U, S=S, ns=ns, cls=i32(cls), ptr=i32(ptr), col=i32(col), col_cls=i32(col_cls),
                bits=torch.from_numpy(bits.view(np.int32)).to(DEV), slot=torch.from_numpy(slot).to(DEV),
                table=torch.randn(U, 64, generator=g).to(DEV), ytab=torch.randn(n_tab, 64, generator=g).to(DEV),
                planes=ops.split_f16_planes((torch.randn(3 * 64, 64, generator=g) / 12).t().contiguous().to(DEV)),
                bias=torch.randn(64, generator=g).to(DEV))


def _launch(c, x, col, self_index, store=True, row0=0):
    out = torch.full((c["N"] + 1, 64), NAN, device=DEV) if store else None
    part = torch.full((c["ns"] + 1, 64), NAN, device=DEV)
    ops.shmp_layer(x, c["ptr"], col, row0, c["N"] - row0, c["S"], 2, c["planes"], c["bias"], out, ytab=c["ytab"],
                   ytab_row0=c["N"], pool=(c["bits"], c["slot"], part), table_empty=1, self_index=self_index)
    return out, part


_SWEEP = [int(v) for v in P.layout("sweep33")]                # segments of 1 .. 33 rows, each at every tile alignment
# one row .. a tail tile .. a second tile (a wave claims two tiles at once: the second one's ids arrive through the
# LDS-direct prefetch, the first one's by plain loads); 600 rows: the waves of a block that win the hand-out take two tiles.
# A THIRD tile per wave -- two flips of the double buffer: ids sent into the half that the first tile's plain loads filled, and
# read there -- needs a third block tile for some block.  The grid is persistent (one block per CU, 256 at most), a block's
# 12 waves claim sub-tiles 0 .. 23 (its first two block tiles, 256 apart) at the start, so sub-tile 24 exists only past
# 2 x 256 x 192 = 98 304 rows: 100 800 rows give 13 blocks a third block tile, and the heavy row and the dense tile lie in it.
CASES = [(f"n{n} u{u}", [n], u, {}) for n in (1, 15, 16, 17, 49) for u in (1, 2, 300)] + \
        [("n600 u300", [600], 300, {}), ("n600 u2", [20] * 30, 2, {}),
         ("sweep33 u300", _SWEEP, 300, {}), ("sweep33 head u1", _SWEEP[:160], 1, {}),
         ("25 sources u300", [7] * 30, 300, dict(heavy_row=37)),
         ("224 ids in a tile u300", [33] * 12, 300, dict(dense_tile=3)),
         ("three tiles per wave u300", [24] * 4200, 300, dict(heavy_row=99000, dense_tile=6190))]


@pytest.mark.parametrize("name,seg_lens,U,kw", CASES, ids=[c[0] for c in CASES])
def test_selfidx_launch_is_the_plain_launch_on_the_materialised_rows(name, seg_lens, U, kw):
    c = _case(seg_lens, U, 200 + len(seg_lens) + U, **kw)
    N, ns, cls = c["N"], c["ns"], c["cls"]
    ref, ref_part = _launch(c, c["table"][cls.long()].contiguous(), c["col"], None)
    assert not torch.isnan(ref[:N]).any() and not torch.isnan(ref_part[:ns]).any()
    out, part = _launch(c, c["table"], c["col_cls"], cls)
    assert torch.equal(out[:N], ref[:N]) and torch.equal(part[:ns], ref_part[:ns])
    assert torch.isnan(out[N:]).all() and torch.isnan(part[ns:]).all()                    # nothing past the end
    # out = None: the partials alone
    _, part2 = _launch(c, c["table"], c["col_cls"], cls, store=False)
    assert torch.equal(part2[:ns], ref_part[:ns]) and torch.isnan(part2[ns:]).all()
    if N > 16:
        # a launch that starts at the second tile: self_index is addressed by the global row id
        ref16, _ = _launch(c, c["table"][cls.long()].contiguous(), c["col"], None, row0=16)
        out16, _ = _launch(c, c["table"], c["col_cls"], cls, row0=16)
        assert torch.isnan(out16[:16]).all() and torch.equal(out16[16:N], ref16[16:N]) and torch.equal(out16[16:N], ref[16:N])


# ---- (d) argument errors -------------------------------------------------------------------------------------------------------
def test_argument_errors_are_einval():
    L = _lib.lib()
    c = _case([5, 12], 3, 1)
    N, ns = c["N"], c["ns"]
    out = torch.full((N, 64), NAN, device=DEV)
    part = torch.full((ns, 64), NAN, device=DEV)
    other = torch.zeros((N, 64), device=DEV)
    p = lambda t: t.data_ptr()    # noqa: E731
    good = dict(x=p(c["table"]), ldx=64, ptr=p(c["ptr"]), col=p(c["col_cls"]), row0=0, n=N, S=4, sm=2, st=2,
                w=p(c["planes"].planes), ws=p(c["planes"].scale), bias=p(c["bias"]), ytab=p(c["ytab"]), ldy=64, y0=N,
                out=p(out), ldo=64, out2=None, ldo2=0, amax=None, xself=None, ldxs=0, bits=p(c["bits"]), slot=p(c["slot"]),
                part=p(part), coef=None, tem=1, idx=p(c["cls"]))

    def call(**kw):
        a = dict(good, **kw)
        return L.desco_shmp_layer_selfidx_f16x3_f32(*[a[k] for k in good], None)

    for kw, why in ((dict(idx=None), b"self_idx is null"),
                    (dict(xself=p(other), ldxs=64), b"excludes xself and self_coef"),
                    (dict(coef=p(other)), b"excludes xself and self_coef"),
                    (dict(part=None), b"pooling index"), (dict(bits=None), b"pooling index"), (dict(slot=None), b"pooling index"),
                    (dict(ldx=128), b"strides other than 64"), (dict(ldy=128), b"strides other than 64"),
                    (dict(ldo=128), b"strides other than 64"),
                    (dict(tem=0), b"one table slot asserted empty"), (dict(tem=3), b"one table slot asserted empty"),
                    (dict(ws=None), b"w_scale is null")):
        assert call(**kw) == -1, kw
        err = L.desco_last_error()
        assert b"desco_shmp_layer_selfidx_f16x3_f32" in err and why in err, (kw, err)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(part).all()                     # refused before any launch
    with pytest.raises(ValueError, match="self_index"):                           # (the wrapper: pooled launches only)
        ops.shmp_layer(c["table"], c["ptr"], c["col_cls"], 0, N, 4, 2, c["planes"], c["bias"], out, ytab=c["ytab"],
                       ytab_row0=N, table_empty=1, self_index=c["cls"])
    assert call() == 0
    torch.cuda.synchronize()
    ref, ref_part = _launch(c, c["table"][c["cls"].long()].contiguous(), c["col"], None)
    assert torch.equal(out, ref[:N]) and torch.equal(part, ref_part[:ns])


# ---- (b), (c) the pass: switch on against switch off ----------------------------------------------------------------------------
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


def _batch(graphs, min_rows_per_class=None, gather_min_rows=0):
    gs = graphs if isinstance(graphs, GraphSet) else GraphSet.from_edge_lists(graphs)
    b = NeighborhoodBatch(build_partition(gs, 4), DEV)
    if min_rows_per_class is not None:
        b.LAYER2_MIN_ROWS_PER_CLASS = min_rows_per_class
    b.LAYER2_GATHER_MIN_ROWS = gather_min_rows
    return b


def _pass(nm, batch, on):
    """(logits, the ``out`` arguments of the table_rows_pool calls, kernel names) of one inference pass"""
    outs = []
    real_rows = ops.table_rows_pool

    def spy_rows(table, cls, n, out, pool):
        outs.append(out)
        real_rows(table, cls, n, out, pool)

    old = GM.SECOND_LAYER_GATHER
    GM.SECOND_LAYER_GATHER, ops.table_rows_pool = on, spy_rows
    ops.PROFILER.reset()
    ops.PROFILER.enabled = True
    try:
        out = nm.graph_to_count(batch).clone()
        torch.cuda.synchronize()
        names = [r[0] for r in ops.PROFILER.records]
    finally:
        GM.SECOND_LAYER_GATHER, ops.table_rows_pool = old, real_rows
        ops.PROFILER.enabled = False
        ops.PROFILER.reset()
    return out, outs, names


ELIGIBLE = {"mutag24": lambda: _batch(synthetic.mutag_shaped(24), 1),
            "mutag24 x4": lambda: _batch(synthetic.mutag_shaped(24).replicate(4)),      # (the default bounds)
            "small": lambda: _batch(SMALL, 1)}


@pytest.mark.parametrize("layers", [8, 3])
@pytest.mark.parametrize("name", list(ELIGIBLE))
def test_eligible_batch_gathers_from_the_table_and_changes_no_bit(models, name, layers):
    """L = 8: the SELFIDX launch stores X_3's rows; L = 3: it is the last layer and stores none"""
    nm, batch = models[layers], ELIGIBLE[name]()
    assert batch.layer2_table_index() is not None
    nm.graph_to_count(batch)                 # (the first pass of a model also folds and splits its weights)
    on, outs_on, names_on = _pass(nm, batch, True)
    off, outs_off, names_off = _pass(nm, batch, False)
    assert torch.isfinite(on).all() and torch.equal(on, off)
    assert len(outs_on) == 1 and outs_on[0] is None                       # the partial sums alone: X_2 is not written
    assert len(outs_off) == 1 and outs_off[0] is not None
    assert names_on.count(SELFIDX) == 1 and SELFIDX not in names_off
    assert names_on.count(PLAIN) == names_off.count(PLAIN) - 1
    # the same launches in the same order, the third layer's count launch under its other name
    i = [k for k, (a, b) in enumerate(zip(names_on, names_off)) if a != b]
    assert len(names_on) == len(names_off) and len(i) == 1 and (names_on[i[0]], names_off[i[0]]) == (SELFIDX, PLAIN)


def test_a_block_at_the_default_bounds_takes_the_path(models):
    """nothing lowered: the 24-graph set x94 has 262 730 count rows (>= 2^18) in 360 classes"""
    nm = models[8]
    batch = NeighborhoodBatch(build_partition(synthetic.mutag_shaped(24).replicate(94), 4), DEV)
    assert batch.num_count >= NeighborhoodBatch.LAYER2_GATHER_MIN_ROWS == batch.LAYER2_GATHER_MIN_ROWS
    assert batch.layer2_table_index() is not None
    nm.graph_to_count(batch)
    on, outs_on, names_on = _pass(nm, batch, True)
    off, outs_off, names_off = _pass(nm, batch, False)
    assert torch.isfinite(on).all() and torch.equal(on, off)
    assert outs_on == [None] and len(outs_off) == 1 and outs_off[0] is not None
    assert names_on.count(SELFIDX) == 1 and SELFIDX not in names_off and names_on.count(PLAIN) == names_off.count(PLAIN) - 1


def test_a_block_below_the_row_bound_keeps_its_rows(models):
    """NeighborhoodBatch.LAYER2_GATHER_MIN_ROWS: at the default bound the small blocks launch what they launch with the switch
    off; a bound equal to the block's count rows takes the path, one more does not"""
    nm = models[8]
    for bound, taken in ((None, False), ("nc", True), ("nc + 1", False)):
        batch = _batch(synthetic.mutag_shaped(24), 1, gather_min_rows=NeighborhoodBatch.LAYER2_GATHER_MIN_ROWS)
        assert NeighborhoodBatch.LAYER2_GATHER_MIN_ROWS == 1 << 18 > batch.num_count
        if bound is not None:
            batch.LAYER2_GATHER_MIN_ROWS = batch.num_count + (bound == "nc + 1")
        nm.graph_to_count(batch)
        on, outs_on, names_on = _pass(nm, batch, True)
        off, _, names_off = _pass(nm, batch, False)
        assert torch.equal(on, off) and (names_on.count(SELFIDX) == 1) == taken and (outs_on == [None]) == taken
        assert taken or names_on == names_off


@pytest.mark.parametrize("name", list(ELIGIBLE))
def test_two_layer_model_is_unchanged(models, name):
    nm, batch = models[2], ELIGIBLE[name]()
    nm.graph_to_count(batch)
    on, outs_on, names_on = _pass(nm, batch, True)
    off, outs_off, names_off = _pass(nm, batch, False)
    assert names_on == names_off and SELFIDX not in names_on and names_on.count("table_rows_pool_kernel") == 1
    assert outs_on == [None] and outs_off == [None]                       # (the second layer is the last: rows never stored)
    assert torch.isfinite(on).all() and torch.equal(on, off)


@pytest.mark.parametrize("name", ["golden", "one neighborhood", "mutag24 default bounds"])
def test_ineligible_batch_launches_the_same_kernels(models, name):
    # (the default bounds refuse the 24-graph set -- 360 classes for 2795 rows --, not the small one: 15 classes for 291 rows)
    batch = {"golden": lambda: _batch(golden_graphs()), "one neighborhood": lambda: _batch([_path(2)]),
             "mutag24 default bounds": lambda: _batch(synthetic.mutag_shaped(24))}[name]()
    assert batch.layer2_table_index() is None
    nm = models[8]
    nm.graph_to_count(batch)
    on, outs_on, names_on = _pass(nm, batch, True)
    off, outs_off, names_off = _pass(nm, batch, False)
    assert sorted(names_on) == sorted(names_off) and names_on == names_off
    assert SELFIDX not in names_on and "table_rows_pool_kernel" not in names_on and not outs_on and not outs_off
    assert torch.isfinite(on).all() and torch.equal(on, off)


def _pipeline(graphs):
    from desco_amd.pipeline import InferencePipeline
    nm, gm = make_models(seed=0)
    nm, gm = nm.to(DEV), gm.to(DEV)
    nm.set_queries(standard_queries()[0])
    pipe = InferencePipeline(nm, gm, graphs if isinstance(graphs, GraphSet) else GraphSet.from_edge_lists(graphs), depth=4,
                             device=DEV)
    for b in pipe.neigh_batches:
        b.LAYER2_MIN_ROWS_PER_CLASS = 1
        b.LAYER2_GATHER_MIN_ROWS = 0
    return pipe


KEYS = ("neigh_count", "node_count", "graph_neigh_count", "graph_gossip_count")


@pytest.mark.parametrize("name", ["mutag24", "small"])
def test_pipeline_outputs_are_equal_with_the_switch_on_and_off(name):
    pipe = _pipeline(synthetic.mutag_shaped(24) if name == "mutag24" else SMALL)
    assert all(b.layer2_table_index() is not None for b in pipe.neigh_batches)
    old = GM.SECOND_LAYER_GATHER
    try:
        res = {}
        for on in (True, False):
            GM.SECOND_LAYER_GATHER = on
            ops.PROFILER.reset()
            ops.PROFILER.enabled = True
            res[on] = {k: v.clone() for k, v in pipe.run().items() if k in KEYS}
            torch.cuda.synchronize()
            res[on]["selfidx"] = [r[0] for r in ops.PROFILER.records].count(SELFIDX)
            ops.PROFILER.enabled = False
    finally:
        GM.SECOND_LAYER_GATHER = old
        ops.PROFILER.enabled = False
        ops.PROFILER.reset()
    assert res[True]["selfidx"] == len(pipe.neigh_batches) and res[False]["selfidx"] == 0
    for k in KEYS:
        assert torch.isfinite(res[True][k]).all() and torch.equal(res[True][k], res[False][k]), k


# ---- (e) capture ----------------------------------------------------------------------------------------------------------------
def test_captured_replay_equals_the_eager_pass():
    assert GM.SECOND_LAYER_GATHER
    pipe = _pipeline(SMALL)
    ops.PROFILER.reset()
    ops.PROFILER.enabled = True
    try:
        eager = {k: v.clone() for k, v in pipe.run().items()}
        torch.cuda.synchronize()
        assert [r[0] for r in ops.PROFILER.records].count(SELFIDX) == len(pipe.neigh_batches)     # the path under test
    finally:
        ops.PROFILER.enabled = False
        ops.PROFILER.reset()
    pipe.capture()
    rep = pipe.run_graph()
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.isfinite(eager[k]).all() and torch.equal(eager[k], rep[k]), k
