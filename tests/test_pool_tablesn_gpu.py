"""desco_table_rows_pooln_f32: the pooled partial sums of ONE TO EIGHT table layers over the same rows -- X_l[i] =
table_l[ids_l[i]] -- from one walk (gnn_model.DEEP_LAYER_TABLES).  Every partial array is compared bit for bit (torch.equal)
with what the single-table launch desco_table_rows_pool_f32 leaves for that table, its ids and the same pooling index: the
rows are the same rows and the running sums the same sums in the same order.  Outputs are pre-filled with NaN."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from desco_amd import _lib, ops  # noqa: E402

import pool_reference as P  # noqa: E402

DEV = "cuda"
NAN = float("nan")
CAP = 624               # table rows of the kernel's LDS budget (asserted equal to the library's: the case ids are built without it)


def _case(seg_lens, U, seed, num_rows=None):
    """N = sum(seg_lens) rows in pooling segments of ``seg_lens`` rows, len(U) random tables of U[k] rows and every row's id in
    each; the first row has id 0 and the last row the last id of every table.  ``num_rows``: the launches run on that prefix
    (the pooling index stays the whole layout's: the prefix's last segment is left open at its end)."""
    g = torch.Generator().manual_seed(seed)
    sp = P.seg_ptr_of(np.asarray(seg_lens, dtype=np.int64))
    N = int(sp[-1])
    n = N if num_rows is None else num_rows
    _, ns, (bits, slot) = P.slots_of(sp, N)
    ids = []
    for u in U:
        i = torch.randint(0, u, (N,), generator=g)
        i[0], i[n - 1] = 0, u - 1
        ids.append(i.to(torch.int32).to(DEV))
    return dict(N=N, n=n, ns=ns, U=U, ids=ids, tables=[torch.randn(u, 64, generator=g).to(DEV) for u in U],
                bits=torch.from_numpy(bits.view(np.int32)).to(DEV), slot=torch.from_numpy(slot).to(DEV))


def _single(c, k, ids=None):
    part = torch.full((c["ns"] + 1, 64), NAN, device=DEV)
    ops.table_rows_pool(c["tables"][k], c["ids"][k] if ids is None else ids, c["n"], None, (c["bits"], c["slot"], part))
    return part


def _walk(c, tables=None, ids=None):
    """through the entry point's own wrapper: one launch for all the layers of the case"""
    t, i = c["tables"] if tables is None else tables, c["ids"] if ids is None else ids
    parts = [torch.full((c["ns"] + 1, 64), NAN, device=DEV) for _ in t]
    ops._table_rows_pooln(list(zip(t, i, parts)), c["n"], c["bits"], c["slot"])
    return parts


def _same(a, b):
    """bit-equal where b is a number, NaN (untouched) where b is NaN"""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def _check(c):
    refs = [_single(c, k) for k in range(len(c["U"]))]
    used = int(torch.isfinite(refs[0][:, 0]).sum())
    assert 0 < used <= c["ns"] and all(torch.isfinite(r[:used]).all() and torch.isnan(r[used:]).all() for r in refs)
    for k, (part, ref) in enumerate(zip(_walk(c), refs)):
        assert _same(part, ref), k


_SWEEP = [int(v) for v in P.layout("sweep33")]                # segments of 1 .. 33 rows, each at every tile alignment
# a one-row block .. five tiles and one row (ragged last tiles); neighborhoods of 1, 16, 17 and 33 rows (ending inside tiles, on
# tile boundaries, spanning three tiles); the sweep; a prefix that leaves its last segment open; 4 500 tiles, so that some waves
# have a second tile in their group of four (the grid is persistent: 256 blocks of 16 waves at most)
LAYOUTS = [(f"n{n}", [n], None) for n in (1, 15, 16, 17, 33, 16 * 5 + 1)] + \
          [(f"{m}-row neighborhoods", [m] * 37, None) for m in (1, 16, 17, 33)] + \
          [("sweep33", _SWEEP, None), ("open last segment", [5, 33, 20, 7], 5 + 33 + 9), ("open at a tile end", [30, 30], 48),
           ("a second tile per wave", [24] * 3000, None)]
# four layers: one id load; five: the second id load with one layer in it; eight: both loads full, one layer in flight at a time
TABLES = {"4 in lds": (40, 200, 300, 60), "4 mixed": (40, 300, 700, 2000), "5 mixed": (40, 300, 700, 900, 2000),
          "8 mixed": (40, 300, 700, 900, 1100, 1300, 100, 1500), "8 ones": (1,) * 8}


@pytest.mark.parametrize("name,seg_lens,n", LAYOUTS, ids=[c[0] for c in LAYOUTS])
@pytest.mark.parametrize("U", list(TABLES.values()), ids=list(TABLES))
def test_walk_leaves_what_the_single_table_launches_leave(name, seg_lens, n, U):
    _check(_case(seg_lens, U, 300 + len(seg_lens) + sum(U), n))


@pytest.mark.parametrize("nl", range(1, 9))
def test_every_number_of_layers(nl):
    """1 .. 8 layers (each its own instantiation), the first two in LDS"""
    _check(_case(_SWEEP[:200] + [33, 1, 16], (100, 300, 700, 800, 900, 1000, 1100, 1200)[:nl], 900 + nl))


# smallest first while they fit together: each position in turn holds the table that stays in global memory alone, that is staged
# alone, the budget exactly filled and passed by one row, nothing staged, everything staged
SIZES = [(200, 300, 100, 24), (200, 300, 100, 25), (CAP, 1, 1, 1), (1, CAP + 1, 1, 1), (700, 800, 900, 1000), (150, 150, 150, 150),
         (700, 100, 100, 100), (100, 700, 100, 100), (100, 100, 700, 100), (100, 100, 100, 700),
         (100, 700, 800, 900), (700, 100, 800, 900), (700, 800, 100, 900), (700, 800, 900, 100),
         (100, 100, 100, 100, 100, 100, 25, 5000), (5000, 100, 100, 100, 100, 100, 100, 100), (100, 700, 100, 700, 100, 700, 100, 700),
         (700, 100, 700, 100, 700), (100, 700, 800, 900, 200)]


@pytest.mark.parametrize("U", SIZES, ids=[" ".join(f"u{u}" for u in U) for U in SIZES])
def test_tables_beyond_the_lds_budget_are_read_from_global_memory(U):
    assert _lib.lib().desco_table_rows_pool2_lds_bytes() // 256 == CAP and _lib.lib().desco_table_rows_pooln_max_layers() == 8
    _check(_case(_SWEEP[:200] + [33, 1, 16], U, 500 + sum(U)))


def test_strided_tables():
    c = _case(_SWEEP[:120], (300, 250, 700, 50, 900), 77)
    wide = [torch.full((u, 64 * (k + 2)), NAN, device=DEV) for k, u in enumerate(c["U"])]
    views = [w[:, 64 * k:64 * (k + 1)] for k, w in enumerate(wide)]
    for v, t in zip(views, c["tables"]):
        v.copy_(t)
    for k, part in enumerate(_walk(c, tables=views)):
        assert _same(part, _single(c, k)), k


@pytest.mark.parametrize("U", [(300, 250, 60, 10), (625, 700, 5000, 800, 900)], ids=["lds", "global"])
def test_ids_outside_their_table_are_clamped(U):
    """an id outside its table is the caller's error (desco_index_range_check_i32 finds it): the kernel reads the nearest
    table row and writes nothing out of bounds"""
    c = _case(_SWEEP[:60], U, 91)
    ids = [i.clone() for i in c["ids"]]
    ids[0][3], ids[0][40], ids[1][17], ids[1][41], ids[2][5], ids[2][42] = U[0] + 5, -2, -(2 ** 31), 2 ** 31 - 1, U[2], -1
    ids[-1][7], ids[-1][43] = U[-1], -7
    parts = _walk(c, ids=ids)
    for k in range(len(U)):
        assert _same(parts[k], _single(c, k, ids[k].clamp(0, U[k] - 1))), k


def test_the_wrapper_splits_and_refuses():
    """ops.table_rows_pool with three entries of ``pool`` per further layer: one launch up to ops.POOL_WALK_LAYERS layers, a
    second walk beyond; rows are never stored"""
    c = _case(_SWEEP[:150], (40, 300, 700, 900, 1100, 20), 5)
    refs = [_single(c, k) for k in range(6)]
    old = ops.POOL_WALK_LAYERS
    try:
        for per_walk, launches in ((8, 1), (4, 2), (2, 3)):
            ops.POOL_WALK_LAYERS = per_walk
            parts = [torch.full((c["ns"] + 1, 64), NAN, device=DEV) for _ in range(6)]
            pool = (c["bits"], c["slot"], parts[5])
            for k in range(5):
                pool += (c["tables"][k], c["ids"][k], parts[k])
            ops.PROFILER.reset()
            ops.PROFILER.enabled = True
            ops.table_rows_pool(c["tables"][5], c["ids"][5], c["n"], None, pool)
            torch.cuda.synchronize()
            assert len(ops.PROFILER.records) == launches
            ops.PROFILER.enabled = False
            for k in range(6):
                assert _same(parts[k], refs[k]), (per_walk, k)
    finally:
        ops.POOL_WALK_LAYERS = old
        ops.PROFILER.enabled = False
        ops.PROFILER.reset()
    with pytest.raises(ValueError, match="partial sums only"):
        ops.table_rows_pool(c["tables"][5], c["ids"][5], c["n"], torch.empty((c["n"], 64), device=DEV), pool)


def test_argument_errors_are_einval():
    L = _lib.lib()
    NL = 5
    c = _case([5, 12], (3, 4, 5, 6, 7), 1)
    parts = [torch.full((c["ns"], 64), NAN, device=DEV) for _ in range(NL)]
    p = lambda t: t.data_ptr()    # noqa: E731
    good = dict(nl=NL, t=[p(t) for t in c["tables"]], ld=[64] * NL, nt=[3, 4, 5, 6, 7], ids=[p(i) for i in c["ids"]],
                part=[p(t) for t in parts], n=17, bits=p(c["bits"]), slot=p(c["slot"]))

    def call(**kw):
        a = {k: (list(v) if isinstance(v, list) else v) for k, v in good.items()}
        for key, v in kw.items():
            if isinstance(v, tuple):               # (k, value): entry k of a per-table array
                a[key][v[0]] = v[1]
            else:
                a[key] = v
        arr = lambda ct, vals: None if vals is None else (ct * NL)(*vals)    # noqa: E731
        return L.desco_table_rows_pooln_f32(a["nl"], arr(ctypes.c_void_p, a["t"]), arr(ctypes.c_int64, a["ld"]),
                                            arr(ctypes.c_int64, a["nt"]), arr(ctypes.c_void_p, a["ids"]),
                                            arr(ctypes.c_void_p, a["part"]), a["n"], a["bits"], a["slot"], None)

    bad = [dict(nl=0), dict(nl=9), dict(nl=-1), dict(t=None), dict(ld=None), dict(nt=None), dict(ids=None), dict(part=None),
           dict(bits=None), dict(slot=None), dict(n=-1)]
    for k in range(NL):
        bad += [dict(t=(k, None)), dict(ids=(k, None)), dict(part=(k, None)), dict(nt=(k, 0)), dict(nt=(k, 2 ** 31)),
                dict(ld=(k, 32)), dict(ld=(k, 66)), dict(t=(k, good["t"][k] + 4)), dict(part=(k, good["part"][k] + 4)),
                dict(part=(k, good["part"][(k + 1) % NL]))]
    for kw in bad:
        assert L.desco_rng_next(None, None, None) == -1          # (another entry point's message in between)
        assert call(**kw) == -1, kw
        assert b"desco_table_rows_pooln_f32" in L.desco_last_error(), (kw, L.desco_last_error())
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in parts)              # refused before any launch
    assert call(n=0) == 0                                        # nothing to do
    assert call() == 0
    torch.cuda.synchronize()
    for k in range(NL):
        assert torch.equal(parts[k], _single(c, k)[:c["ns"]]), k
