"""gnn_model.SECOND_LAYER_TABLE: the second layer's count launch on one representative per class of rows
(NeighborhoodBatch.layer2_table_index), the rows and their pooled partial sums from the table of the representatives' rows
(desco_table_rows_pool_f32).  Everything here is a bit-for-bit comparison (torch.equal): the layer kernel's arithmetic is
row-local, so a representative's row IS the row of every member of its class, and the running sums are the same sums in
the same order.

The index refuses a block with fewer than 8 rows per class (a bound on the profit); the small blocks here lower it on their
own batch object so that the path is taken."""
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
from helpers import golden_graphs, make_models, standard_queries  # noqa: E402

DEV = "cuda"
NAN = float("nan")


def _path(n):
    return (n, [(i, i + 1) for i in range(n - 1)])


def _ring(n):
    return (n, [(i, (i + 1) % n) for i in range(n)])


def _star(k):
    return (k + 1, [(0, v) for v in range(1, k + 1)])


SMALL = ([_path(n) for n in range(2, 8)] + [_ring(5), _ring(6)] + [_star(k) for k in range(1, 5)]) * 3


@pytest.fixture(scope="module")
def model():
    nm, _ = make_models(seed=0)
    qids, _ = standard_queries()
    nm = nm.to(DEV)
    nm.set_queries(qids)
    return nm


def _batch(graphs, min_rows_per_class=None):
    gs = graphs if isinstance(graphs, GraphSet) else GraphSet.from_edge_lists(graphs)
    b = NeighborhoodBatch(build_partition(gs, 4), DEV)
    if min_rows_per_class is not None:
        b.LAYER2_MIN_ROWS_PER_CLASS = min_rows_per_class
    return b


# ---- (a) desco_table_rows_pool_f32 against the layer kernel's pooled launch on the same rows -----------------------------
def _class_case(seg_lens, U, seed):
    """N = sum(seg_lens) count rows in segments of ``seg_lens`` rows, each row a copy of one of U prototype rows (slot
    degrees and source ids): the full 4-slot CSR, the compact CSR of the prototypes and the rows' classes.  Table slot 0
    (CSR slot 2) is empty, a prototype has at most 7 sources, the LAST class belongs to the last row alone."""
    g = torch.Generator().manual_seed(seed)
    S, n_x, n_tab = 4, 23, 11
    sp = P.seg_ptr_of(np.asarray(seg_lens, dtype=np.int64))
    N = int(sp[-1])
    cnt = torch.randint(0, 4, (U, S), generator=g)
    cnt[:, 2] = 0
    cnt[:, 3] = torch.randint(0, 2, (U,), generator=g)
    cnt[::5] = 0                                                          # prototypes without any source
    cnt[1::5, :2] = 0                                                     # ... and with a table source alone
    seg = [[int(v) for s in range(S) for v in torch.randint(0, n_tab if s == 3 else n_x, (int(cnt[u, s]),), generator=g)]
           for u in range(U)]
    cls = torch.randint(0, max(U - 1, 1), (N,), generator=g)
    cls[N - 1] = U - 1
    rep_ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(cnt.reshape(-1), 0)])
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(cnt[cls].reshape(-1), 0)])
    col = [v for c in cls.tolist() for v in seg[c]]
    rep_col = [v for s in seg for v in s]
    _, ns, (bits, slot) = P.slots_of(sp, N)
    nt = (U + 15) // 16
    rep_bits = np.zeros(nt, np.int32)
    rep_bits[-1] = 1 << ((U - 1) % 16)
    i32 = lambda a: torch.as_tensor(a, dtype=torch.int32).reshape(-1).to(DEV)    # noqa: E731
    return dict(N=N, U=U, S=S, ns=ns, cls=i32(cls), ptr=i32(ptr), col=i32(col), rep_ptr=i32(rep_ptr), rep_col=i32(rep_col),
                bits=torch.from_numpy(bits.view(np.int32)).to(DEV), slot=torch.from_numpy(slot).to(DEV),
                rep_bits=torch.from_numpy(rep_bits).to(DEV), rep_slot=torch.arange(nt, dtype=torch.int32, device=DEV),
                x=torch.randn(n_x, 64, generator=g).to(DEV), ytab=torch.randn(n_tab, 64, generator=g).to(DEV),
                planes=ops.split_f16_planes((torch.randn(3 * 64, 64, generator=g) / 12).t().contiguous().to(DEV)),
                bias=torch.randn(64, generator=g).to(DEV), coef=(torch.randn(S + 1, 64, generator=g) / 4).to(DEV))


def _layer(c, ptr, col, n, bits, slot, ns):
    out = torch.full((n, 64), NAN, device=DEV)
    part = torch.full((ns, 64), NAN, device=DEV)
    ops.shmp_layer(c["x"], ptr, col, 0, n, c["S"], 2, c["planes"], c["bias"], out, ytab=c["ytab"], ytab_row0=0,
                   pool=(bits, slot, part), self_coef=c["coef"], table_empty=1)
    return out, part


_SWEEP = [int(v) for v in P.layout("sweep33")]                # segments of 1 .. 33 rows, each at every tile alignment
CLASS_CASES = [(f"n{n} u{u}", [n], u) for n in (1, 15, 16, 17, 49) for u in (1, 2, 300)] + \
              [("sweep33 u300", _SWEEP, 300), ("sweep33 head u2", _SWEEP[:160], 2), ("ones u300", [1] * 100, 300),
               ("1..33 u300", list(range(1, 34)) + list(range(33, 0, -1)), 300)]


@pytest.mark.parametrize("name,seg_lens,U", CLASS_CASES, ids=[c[0] for c in CLASS_CASES])
def test_table_rows_and_partials_are_the_pooled_layer_launchs(name, seg_lens, U):
    c = _class_case(seg_lens, U, 100 + len(seg_lens) + U)
    ref, ref_part = _layer(c, c["ptr"], c["col"], c["N"], c["bits"], c["slot"], c["ns"])
    assert not torch.isnan(ref).any() and not torch.isnan(ref_part).any()
    table, _ = _layer(c, c["rep_ptr"], c["rep_col"], U, c["rep_bits"], c["rep_slot"], (U + 15) // 16)
    assert not torch.isnan(table).any()
    assert torch.equal(table[c["cls"].long()], ref)                       # the layer's rows are a function of the class
    out = torch.full((c["N"] + 1, 64), NAN, device=DEV)
    part = torch.full((c["ns"] + 1, 64), NAN, device=DEV)
    ops.table_rows_pool(table, c["cls"], c["N"], out, (c["bits"], c["slot"], part))
    assert torch.equal(out[:c["N"]], ref) and torch.equal(part[:c["ns"]], ref_part)
    assert torch.isnan(out[c["N"]:]).all() and torch.isnan(part[c["ns"]:]).all()          # nothing past the end
    # out = NULL: the partials alone
    part2 = torch.full((c["ns"] + 1, 64), NAN, device=DEV)
    ops.table_rows_pool(table, c["cls"], c["N"], None, (c["bits"], c["slot"], part2))
    assert torch.equal(part2[:c["ns"]], ref_part) and torch.isnan(part2[c["ns"]:]).all()
    # a table with a wider row stride, rows into a column block of a wider tensor
    wide = torch.full((U, 128), NAN, device=DEV)
    wide[:, :64] = table
    out3 = torch.full((c["N"], 192), NAN, device=DEV)
    ops.table_rows_pool(wide[:, :64], c["cls"], c["N"], out3[:, 64:128], (c["bits"], c["slot"], part2))
    assert torch.equal(out3[:, 64:128], ref) and torch.isnan(out3[:, :64]).all() and torch.isnan(out3[:, 128:]).all()
    assert torch.equal(part2[:c["ns"]], ref_part)


# ---- (b), (c) the pass: switch on against switch off ---------------------------------------------------------------------
def _pass(nm, batch, on):
    """(logits, X_2's count rows, pool_parts[2], kernel names) of one inference pass"""
    got = {}
    real_layer, real_rows = ops.shmp_layer, ops.table_rows_pool
    nc = batch.num_count

    def spy_layer(*a, **kw):
        r = real_layer(*a, **kw)
        if kw.get("self_coef") is not None and a[4] == nc and "x2" not in got:      # the l = 1 count launch on all rows
            got["x2"], got["part"] = a[9][:nc].clone(), kw["pool"][2].clone()
        return r

    def spy_rows(table, cls, n, out, pool):
        real_rows(table, cls, n, out, pool)
        got["x2"], got["part"], got["u2"] = out[:n].clone(), pool[2].clone(), table.shape[0]

    old = GM.SECOND_LAYER_TABLE
    GM.SECOND_LAYER_TABLE, ops.shmp_layer, ops.table_rows_pool = on, spy_layer, spy_rows
    ops.PROFILER.reset()
    ops.PROFILER.enabled = True
    try:
        out = nm.graph_to_count(batch).clone()
        torch.cuda.synchronize()
        names = [r[0] for r in ops.PROFILER.records]
    finally:
        GM.SECOND_LAYER_TABLE, ops.shmp_layer, ops.table_rows_pool = old, real_layer, real_rows
        ops.PROFILER.enabled = False
        ops.PROFILER.reset()
    return out, got, names


@pytest.mark.parametrize("name", ["mutag24", "mutag24 x4", "small"])
def test_eligible_batch_takes_the_table_path_and_changes_no_bit(model, name):
    batch = {"mutag24": lambda: _batch(synthetic.mutag_shaped(24), 1),
             "mutag24 x4": lambda: _batch(synthetic.mutag_shaped(24).replicate(4)),      # (the default bounds)
             "small": lambda: _batch(SMALL, 1)}[name]()
    idx = batch.layer2_table_index()
    assert idx is not None
    ops.index_range_check(idx[0], (idx[1].numel() - 1) // 4)
    model.graph_to_count(batch)              # (the first pass of a model also folds and splits its weights)
    on, got_on, names_on = _pass(model, batch, True)
    off, got_off, names_off = _pass(model, batch, False)
    assert got_on["u2"] == (idx[1].numel() - 1) // 4 < batch.num_count and "u2" not in got_off
    assert torch.isfinite(got_off["x2"]).all() and torch.equal(got_on["x2"], got_off["x2"])
    assert torch.equal(got_on["part"], got_off["part"])
    assert torch.isfinite(on).all() and torch.equal(on, off)
    # the same launches but one more: the count launch of layer 2 (on the representatives) and the rows' kernel
    i = [k for k, n in enumerate(names_off) if n.endswith(",selfdeg>")][0]
    assert names_on == names_off[:i + 1] + ["table_rows_pool_kernel"] + names_off[i + 1:]


@pytest.mark.parametrize("name", ["golden", "one neighborhood", "mutag24 default bounds"])
def test_ineligible_batch_launches_the_same_kernels(model, name):
    batch = {"golden": lambda: _batch(golden_graphs()), "one neighborhood": lambda: _batch([_path(2)]),
             "mutag24 default bounds": lambda: _batch(synthetic.mutag_shaped(24))}[name]()
    assert batch.layer2_table_index() is None
    model.graph_to_count(batch)              # (the first pass of a model also folds and splits its weights)
    on, got_on, names_on = _pass(model, batch, True)
    off, got_off, names_off = _pass(model, batch, False)
    assert names_on == names_off and "table_rows_pool_kernel" not in names_on and "u2" not in got_on
    assert torch.isfinite(on).all() and torch.equal(on, off)
    if "x2" in got_on:
        assert torch.equal(got_on["x2"], got_off["x2"]) and torch.equal(got_on["part"], got_off["part"])


# ---- (e) argument errors ------------------------------------------------------------------------------------------------------
def test_argument_errors_are_einval():
    L = _lib.lib()
    c = _class_case([5, 12], 3, 1)
    table = torch.randn(3, 64, device=DEV)
    out = torch.full((17, 64), NAN, device=DEV)
    part = torch.full((c["ns"], 64), NAN, device=DEV)
    good = dict(table=table.data_ptr(), ldt=64, nt=3, cls=c["cls"].data_ptr(), n=17, out=out.data_ptr(), ldo=64,
                bits=c["bits"].data_ptr(), slot=c["slot"].data_ptr(), part=part.data_ptr())

    def rows(**kw):
        a = dict(good, **kw)
        return L.desco_table_rows_pool_f32(a["table"], a["ldt"], a["nt"], a["cls"], a["n"], a["out"], a["ldo"], a["bits"],
                                           a["slot"], a["part"], None)

    for kw in (dict(table=None), dict(cls=None), dict(bits=None), dict(slot=None), dict(part=None), dict(n=-1), dict(nt=0),
               dict(ldt=32), dict(ldt=66), dict(table=good["table"] + 4), dict(out=good["out"] + 4), dict(ldo=66),
               dict(part=good["part"] + 4), dict(out=good["table"])):
        assert rows(**kw) == -1, kw
        assert b"desco_table_rows_pool_f32" in L.desco_last_error(), (kw, L.desco_last_error())
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(part).all()                     # refused before any launch
    # an index outside the table: found by the range check (the rows' kernel itself never reads out of bounds)
    ops.index_range_check(c["cls"], 3)
    for bad in (3, -1):
        cls = c["cls"].clone()
        cls[16] = bad
        with pytest.raises(RuntimeError, match="outside the table"):
            ops.index_range_check(cls, 3)
    with pytest.raises(RuntimeError, match="outside the table"):
        ops.index_range_check(c["cls"], 2)
    scratch = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert L.desco_index_range_check_i32(None, 4, 4, scratch.data_ptr(), None) == -1
    assert L.desco_index_range_check_i32(c["cls"].data_ptr(), 4, 4, None, None) == -1
    assert rows() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, table[c["cls"].long()])
