"""Host side of gnn_model.TABLE_NARROW: NeighborhoodBatch.table_empty and canonical_table_index on CPU tensors, and the
argument check of desco_shmp_layer_narrow_f16x3_f32 (no launch: the library is only loaded)."""
import numpy as np
import torch

from desco_amd import _lib
from desco_amd.batch import NeighborhoodBatch
from desco_amd.graphs import GraphSet
from desco_amd.partition import build_partition


def _path(n):
    return (n, [(i, i + 1) for i in range(n - 1)])


def _ring(n):
    return (n, [(i, (i + 1) % n) for i in range(n)])


def _star(k):
    return (k + 1, [(0, v) for v in range(1, k + 1)])


FREE = [_path(n) for n in (2, 3, 7)] + [_ring(5), _ring(6)] + [_star(k) for k in (1, 4, 17)]
TRIANGLE = (3, [(0, 1), (1, 2), (0, 2)])


def _batch(graphs):
    return NeighborhoodBatch(build_partition(GraphSet.from_edge_lists(graphs), 4), "cpu")


def test_table_empty_is_the_mask_of_the_empty_canonical_to_count_relations():
    """slot = 2 (source is canonical) + tride: a triangle-free block has no entry in CSR slot 2 (table slot 0) and tride
    entries in CSR slot 3; one triangle anywhere clears the bit"""
    free, tri = _batch(FREE), _batch(FREE + [TRIANGLE])
    for b in (free, tri):
        deg = np.diff(np.asarray(b.part.vrowptr, dtype=np.int64)).reshape(-1, 4)[:b.num_count]
        assert b.table_empty == (1 if deg[:, 2].sum() == 0 else 0) | (2 if deg[:, 3].sum() == 0 else 0)
        assert b.table1_empty == bool(b.table_empty & 2)
    assert free.table_empty == 1 and tri.table_empty == 0


def test_canonical_table_index_is_a_faithful_remap_of_the_table_slots():
    b = _batch(FREE + [TRIANGLE])
    S, nc, n = 4, b.num_count, b.num_rows
    uptr_c, canon_id, vcol_tc = (t.numpy().astype(np.int64) for t in b.canonical_table_index())
    vcol_t = b.degree_table_index()[2].numpy().astype(np.int64)
    deg = np.diff(np.asarray(b.part.vrowptr, dtype=np.int64)).reshape(n, S)
    ut = np.diff(uptr_c).reshape(-1, S)
    assert len(np.unique(ut, axis=0)) == len(ut) < n - nc and (ut[canon_id] == deg[nc:]).all()
    vcol = np.asarray(b.part.vcol, dtype=np.int64)
    high = np.repeat(np.arange(n * S) % S, deg.reshape(-1)) >= 2
    assert high.any() and (vcol[high] >= nc).all()
    # any canonical rows that are a function of the tuple: gathers through the table equal gathers through the rows
    T = np.random.default_rng(0).standard_normal((len(ut), 3))
    assert np.array_equal(T[vcol_tc[high]], T[canon_id][vcol[high] - nc])
    assert np.array_equal(vcol_tc[~high], vcol_t[~high])


def test_narrow_entry_point_validates_its_arguments():
    """a [n, 64] table with two table slots needs a slot asserted empty; the mask has two bits and needs slots_table == 2
    (fake aligned host pointers, never dereferenced: every call is refused before any HIP call)"""
    L = _lib.lib()
    buf = np.zeros(64 * 1024, np.float32)
    idx = np.zeros(64, np.int32)
    p, q = buf.ctypes.data, idx.ctypes.data
    o, t, w = p + 65536, p + 131072, p + 196608

    def narrow(st=2, ldy=64, mask=0):
        return L.desco_shmp_layer_narrow_f16x3_f32(p, 64, q, q, 0, 8, 4, 2, st, w, w, w, t, ldy, 0, o, 64, None, 0, None,
                                                   None, 0, None, None, None, None, mask, None)

    for kw in (dict(), dict(mask=4), dict(mask=-1), dict(st=1, mask=1), dict(ldy=32, mask=1)):
        assert L.desco_rng_next(None, None, None) == -1          # (another entry point's message in between)
        assert narrow(**kw) == -1, kw
        assert b"desco_shmp_layer_narrow_f16x3_f32" in L.desco_last_error(), (kw, L.desco_last_error())
    assert L.desco_shmp_layer_f16x3_f32(p, 64, q, q, 0, 8, 4, 2, 2, w, w, w, t, 64, 0, o, 64, None, 0, None, None, 0,
                                        None) == -1
    assert b"desco_shmp_layer_f16x3_f32" in L.desco_last_error()
