"""gnn_model.TABLE_NARROW: no table columns for an empty canonical->count relation, and the second layer's table from the
distinct canonical degree tuples.  Everything here is a bit-for-bit comparison (torch.equal) -- the narrow path reads
the same values into the same sums in the same order as the [B, 128] table product it replaces.

The relation slots are  slot = 2 (source is canonical) + tride  (partition.py): the canonical->count TRIANGLE relation
is CSR slot 2 = table slot 0, the tride relation CSR slot 3 = table slot 1.  A triangle-free batch therefore has table
slot 0 empty (NeighborhoodBatch.table_empty == 1) and its narrow table is the product with the SECOND 64-row block of
wt_tab_l64; the layer kernel takes a mask of the empty table slots, so both halves are covered below."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import desco_amd.gnn_model as GM  # noqa: E402
from desco_amd import _lib, ops  # noqa: E402
from desco_amd.batch import NeighborhoodBatch  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402
from desco_amd.partition import build_partition  # noqa: E402

import pool_reference as P  # noqa: E402
from helpers import make_models, standard_queries  # noqa: E402

DEV = "cuda"
NAN = float("nan")


def _path(n):
    return (n, [(i, i + 1) for i in range(n - 1)])


def _ring(n):
    return (n, [(i, (i + 1) % n) for i in range(n)])


def _star(k):
    return (k + 1, [(0, v) for v in range(1, k + 1)])


# paths, a 5-ring, a 6-ring and stars: no triangle; the hub neighborhoods of the stars have 1 .. 33 count rows
TRIANGLE_FREE = [_path(n) for n in (2, 3, 7, 12)] + [_ring(5), _ring(6)] + [_star(k) for k in range(1, 34)]
TRIANGLE = (3, [(0, 1), (1, 2), (0, 2)])


@pytest.fixture(scope="module")
def model():
    nm, _ = make_models(seed=0)
    qids, _ = standard_queries()
    nm = nm.to(DEV)
    nm.set_queries(qids)
    return nm


def _batch(graphs):
    return NeighborhoodBatch(build_partition(GraphSet.from_edge_lists(graphs), 4), DEV)


def _logits(nm, batch, narrow):
    """(logits, [(ytab shape, ytab_row0, table_empty)] of the count-row launches) of one inference pass"""
    calls = []
    real = ops.shmp_layer

    def spy(*a, **kw):
        if kw.get("ytab") is not None:
            calls.append((tuple(kw["ytab"].shape), kw.get("ytab_row0", 0), kw.get("table_empty", 0)))
        return real(*a, **kw)

    old = GM.TABLE_NARROW
    GM.TABLE_NARROW, ops.shmp_layer = narrow, spy
    try:
        out = nm.graph_to_count(batch).clone()
    finally:
        GM.TABLE_NARROW, ops.shmp_layer = old, real
    return out, calls


def test_triangle_free_batch_takes_the_narrow_path_and_changes_no_bit(model):
    batch = _batch(TRIANGLE_FREE)
    sizes = np.diff(np.asarray(batch.part.count_ptr))
    assert set(sizes.tolist()) >= set(range(1, 34)) and sizes.max() == 33      # every tile alignment, ragged last tiles
    assert batch.table_empty == 1 and not batch.table1_empty                   # no triangle relation, tride edges present
    B, nc = batch.num_graphs, batch.num_count
    ctab = batch.canonical_table_index()
    assert ctab is not None
    uc = (ctab[0].numel() - 1) // batch.slots
    assert 1 <= uc <= 16 < B
    on, calls_on = _logits(model, batch, True)
    off, calls_off = _logits(model, batch, False)
    L = model.emb_model.gnn_core.layer_num
    assert len(calls_on) == len(calls_off) == L - 1
    assert all(shape == (B, 128) and r0 == nc and tem == 0 for shape, r0, tem in calls_off)
    assert calls_on[0] == ((uc, 64), 0, 1)                                     # layer 2: the table of the distinct tuples
    assert all(c == ((B, 64), nc, 1) for c in calls_on[1:])
    assert torch.isfinite(on).all() and torch.equal(on, off)


def test_single_neighborhood_batch(model):
    batch = _batch([_path(2)])
    assert batch.num_graphs == 1 and batch.table_empty == 1
    on, calls = _logits(model, batch, True)
    off, _ = _logits(model, batch, False)
    assert calls[0] == ((1, 64), 0, 1) and all(c == ((1, 64), batch.num_count, 1) for c in calls[1:])
    assert torch.isfinite(on).all() and torch.equal(on, off)


def test_one_triangle_keeps_the_wide_path(model):
    batch = _batch(TRIANGLE_FREE + [TRIANGLE])
    assert batch.table_empty == 0
    on, calls = _logits(model, batch, True)
    off, _ = _logits(model, batch, False)
    assert all(shape == (batch.num_graphs, 128) and r0 == batch.num_count and tem == 0 for shape, r0, tem in calls)
    assert torch.isfinite(on).all() and torch.equal(on, off)


# ---- the layer kernel's entry point alone -----------------------------------------------------------------------------
def _layer_case(empty_slot, seed):
    """a count-row launch on a random 4-slot CSR whose table slot ``empty_slot`` has no entry: rows in segments of 1 .. 33
    rows (several block tiles, a ragged last tile); a few rows hold several sources in the live table slot (the
    cooperative path reads the table too)"""
    g = torch.Generator().manual_seed(seed)
    sp = P.seg_ptr_of(P.layout("sweep33"))
    N, S, sm, n_tab = int(sp[-1]), 4, 2, 37
    cnt = torch.randint(0, 4, ((N + n_tab) * S,), generator=g)
    cnt[::7] = 0
    cnt = cnt.view(-1, S)
    live = 1 - empty_slot
    cnt[:, sm + live] = (torch.rand(N + n_tab, generator=g) < 0.4).long()      # canonical->count: one source per row ...
    cnt[5::41, sm + live] = 3                                                   # ... a general input may hold more
    cnt[:, sm + empty_slot] = 0
    cnt = cnt.reshape(-1)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(cnt, 0)])
    col = torch.randint(0, N, (int(ptr[-1]),), generator=g)
    vrow = torch.repeat_interleave(torch.arange((N + n_tab) * S), cnt)
    col = torch.where((vrow % S) >= sm, N + col % n_tab, col).to(torch.int32)
    wide = torch.randn(n_tab, 128, generator=g)
    narrow = wide[:, 64 * live:64 * live + 64].contiguous()
    wide[:, 64 * empty_slot:64 * empty_slot + 64] = NAN
    _, ns, (bits, slot) = P.slots_of(sp, N)
    return dict(N=N, S=S, sm=sm, ns=ns, x=torch.randn(N + n_tab, 64, generator=g).to(DEV), ptr=ptr.to(torch.int32).to(DEV),
                col=col.to(DEV), planes=ops.split_f16_planes((torch.randn(3 * 64, 64, generator=g) / 12).t().contiguous().to(DEV)),
                bias=torch.randn(64, generator=g).to(DEV), coef=(torch.randn(S + 1, 64, generator=g) / 4).to(DEV),
                wide=wide.to(DEV), narrow=narrow.to(DEV), bits=torch.from_numpy(bits.view(np.int32)).to(DEV),
                slot=torch.from_numpy(slot).to(DEV))


def _launch(c, form, ytab, mask, x=None):
    out = torch.full((c["N"], 64), NAN, device=DEV)
    part = torch.full((c["ns"], 64), NAN, device=DEV) if form != "plain" else None
    ops.shmp_layer(c["x"] if x is None else x, c["ptr"], c["col"], 0, c["N"], c["S"], c["sm"], c["planes"], c["bias"], out,
                   ytab=ytab, ytab_row0=c["N"], pool=None if part is None else (c["bits"], c["slot"], part),
                   self_coef=c["coef"] if form == "selfdeg" else None, table_empty=mask)
    return out, part


@pytest.mark.parametrize("empty_slot", [1, 0])
@pytest.mark.parametrize("form", ["plain", "pool", "selfdeg"])
def test_layer_kernel_reads_the_narrow_table_bit_for_bit(form, empty_slot):
    """[n, 128] table whose half of the empty slot is NaN (today's launch: nothing asserted) against the [n, 64] table of
    the live slot with the assertion (the kernel's NARROW instantiations); also the wide table WITH the assertion, which
    needs none and runs today's launch"""
    c = _layer_case(empty_slot, 11 + empty_slot)
    mask = 1 << empty_slot
    ref, ref_part = _launch(c, form, c["wide"], 0)
    assert not torch.isnan(ref).any() and (ref_part is None or not torch.isnan(ref_part).any())
    runs = [_launch(c, form, c["narrow"], mask), _launch(c, form, c["wide"], mask)]
    for out, part in runs:
        assert torch.equal(out, ref)
        assert part is None or torch.equal(part, ref_part)


def test_narrow_table_without_the_assertion_is_refused():
    c = _layer_case(1, 3)
    L = _lib.lib()
    out = torch.empty((c["N"], 64), device=DEV)
    head = (c["x"].data_ptr(), 64, c["ptr"].data_ptr(), c["col"].data_ptr(), 0, c["N"], c["S"], c["sm"], 2,
            c["planes"].planes.data_ptr(), c["planes"].scale.data_ptr(), c["bias"].data_ptr(), c["narrow"].data_ptr(), 64,
            c["N"], out.data_ptr(), 64, None, 0, None, None, 0)
    for mask in (0, 4):
        assert L.desco_shmp_layer_narrow_f16x3_f32(*head, None, None, None, None, mask, None) == -1
        assert b"desco_shmp_layer_narrow_f16x3_f32" in L.desco_last_error()
    assert L.desco_shmp_layer_f16x3_f32(*head, None) == -1
    assert b"desco_shmp_layer_f16x3_f32" in L.desco_last_error()
    torch.cuda.synchronize()


# ---- part 2: the second layer's table ------------------------------------------------------------------------------------
def test_layer2_table_rows_are_the_full_products_rows(model):
    batch = _batch(TRIANGLE_FREE)
    S, nc, n, B = batch.slots, batch.num_count, batch.num_rows, batch.num_graphs
    uptr_c, canon_id, vcol_tc = batch.canonical_table_index()
    _, _, vcol_t = batch.degree_table_index()
    # the index: distinct tuples, every canonical row's id points at ITS tuple, the table slots' sources at their row's id
    vr = batch.vrowptr.long()
    deg = (vr[1:] - vr[:-1]).view(n, S)
    ut = (uptr_c.long()[1:] - uptr_c.long()[:-1]).view(-1, S)
    assert len(torch.unique(ut, dim=0)) == len(ut) and torch.equal(ut[canon_id.long()], deg[nc:])
    slot_of = torch.repeat_interleave(torch.arange(n * S, device=DEV) % S, deg.reshape(-1))
    high = slot_of >= 2
    col = batch.vcol.long()
    assert bool(high.any()) and bool((col[high] >= nc).all())
    assert torch.equal(vcol_tc.long()[high], canon_id.long()[col[high] - nc])
    assert torch.equal(vcol_tc[~high], vcol_t[~high])
    # the table: row u is the full l = 1 product's row of every canonical row with tuple u
    gnn = model.emb_model
    pk = gnn.packed()
    x0 = {t: pk["pre"][t][1] for t in ("count", "canonical")}
    coef = GM._first_layer_coef(pk, "canonical", 2, S, x0, lambda t, s: "count" if s < 2 else "canonical", DEV)
    crows = torch.empty((B, 64), device=DEV)
    ops.degree_affine(batch.vrowptr, nc, B, S, coef, ops.ACT_RELU, 0.0, crows, out_row0=0)
    planes = pk["layers"][1]["count"]["wt_tab_l64"]
    full = ops.linear64(crows, planes)                                         # [B, 128]
    for blk in (slice(0, 1), slice(1, 2), slice(0, 2)):
        tab = GM._layer2_table(uptr_c, S, coef, planes[blk])
        assert tab.shape == (len(ut), 64 * (blk.stop - blk.start))
        assert torch.equal(tab[canon_id.long()], full[:, 64 * blk.start:64 * blk.stop])
