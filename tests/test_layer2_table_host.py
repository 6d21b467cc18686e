"""Host side of gnn_model.SECOND_LAYER_TABLE: NeighborhoodBatch.layer2_table_index on CPU tensors against a brute-force
dict over (slot degrees, remapped segment), and the argument checks of the two new entry points (no launch).

The index refuses a block with fewer than 8 rows per class (LAYER2_MIN_ROWS_PER_CLASS: a bound on the profit, not on
correctness), which the small blocks of this file are; they lower it on their own batch object to have the classes built,
and the default is tested as a refusal."""
import numpy as np
import pytest

from desco_amd import _lib, synthetic
from desco_amd.batch import NeighborhoodBatch
from desco_amd.graphs import GraphSet
from desco_amd.partition import build_partition
from helpers import golden_graphs


def _path(n):
    return (n, [(i, i + 1) for i in range(n - 1)])


def _ring(n):
    return (n, [(i, (i + 1) % n) for i in range(n)])


def _star(k):
    return (k + 1, [(0, v) for v in range(1, k + 1)])


TRIANGLE = (3, [(0, 1), (1, 2), (0, 2)])


def _batch(graphs, min_rows_per_class=None):
    gs = graphs if isinstance(graphs, GraphSet) else GraphSet.from_edge_lists(graphs)
    b = NeighborhoodBatch(build_partition(gs, 4), "cpu")
    if min_rows_per_class is not None:
        b.LAYER2_MIN_ROWS_PER_CLASS = min_rows_per_class
    return b


def _brute_force(b):
    """(keys, classes): per count row its (slot degrees, segment of vcol_tc) and the dict key -> rows, in row order"""
    S, nc = 4, b.num_count
    vr = np.asarray(b.part.vrowptr, dtype=np.int64)
    vcol_tc = b.canonical_table_index()[2].numpy().astype(np.int64)
    keys, classes = [], {}
    for i in range(nc):
        k = (tuple(np.diff(vr[S * i:S * i + S + 1]).tolist()), tuple(vcol_tc[vr[S * i]:vr[S * i + S]].tolist()))
        keys.append(k)
        classes.setdefault(k, []).append(i)
    return keys, classes


def _eligible(b):
    """the issue's four conditions, by brute force"""
    if not b.table_empty or b.degree_table_index() is None or b.canonical_table_index() is None:
        return False
    vr = np.asarray(b.part.vrowptr, dtype=np.int64)
    if (vr[4:4 * b.num_count + 1:4] - vr[0:4 * b.num_count:4]).max() > 8:
        return False
    u2 = len(_brute_force(b)[1])
    return u2 <= 16384 and u2 * b.LAYER2_MIN_ROWS_PER_CLASS <= b.num_count


def _check_index(b):
    idx = b.layer2_table_index()
    assert idx is not None and b.layer2_table_index() is idx            # built once, cached
    cls, rep_uptr, rep_vcol, vcol_2 = (t.numpy().astype(np.int64) for t in idx)
    assert all(t.dtype.is_floating_point is False and t.element_size() == 4 for t in idx)
    S, nc, n = 4, b.num_count, b.num_rows
    keys, classes = _brute_force(b)
    u2 = len(classes)
    # cls is consistent: one id per distinct key, ids 0 .. U_2 - 1
    assert cls.shape == (nc,) and sorted(set(cls.tolist())) == list(range(u2))
    assert len({(keys[i], int(cls[i])) for i in range(nc)}) == u2
    # the compact CSR: class c's row is its LOWEST row's degrees and segment, verbatim
    assert rep_uptr.shape == (u2 * S + 1,) and rep_uptr[0] == 0 and rep_vcol.shape == (rep_uptr[-1],)
    for k, rows in classes.items():
        c = int(cls[rows[0]])
        assert rows[0] == min(rows)
        assert tuple(np.diff(rep_uptr[S * c:S * c + S + 1]).tolist()) == k[0]
        assert tuple(rep_vcol[rep_uptr[S * c]:rep_uptr[S * c + S]].tolist()) == k[1]
    # vcol_2: the sources of slots 0 and 1 (count rows) by their class, canonical rows' segments too; slots 2, 3 untouched
    vr = np.asarray(b.part.vrowptr, dtype=np.int64)
    vcol = np.asarray(b.part.vcol, dtype=np.int64)
    low = np.repeat(np.arange(n * S) % S, np.diff(vr)) < 2
    assert vcol_2.shape == vcol.shape and low[vr[S * nc]:].any()
    assert np.array_equal(vcol_2[low], cls[vcol[low]]) and np.array_equal(vcol_2[~low], vcol[~low])
    return u2


@pytest.mark.parametrize("name", ["mutag24", "ring6", "path6", "star4", "mixed"])
def test_layer2_classes_match_a_brute_force_dict(name):
    graphs = {"mutag24": synthetic.mutag_shaped(24), "ring6": [_ring(6)], "path6": [_path(6)], "star4": [_star(4)],
              "mixed": [_ring(6), _path(6), _star(4), _ring(5), _path(3), _ring(6), _star(3)]}[name]
    b = _batch(graphs, min_rows_per_class=1)
    assert _eligible(b)
    u2 = _check_index(b)
    assert 1 <= u2 < b.num_count or b.num_count == 1


def test_layer2_index_with_the_default_bounds():
    """mutag_shaped(24) four times over has 8 rows per class and is taken as it stands; replication adds no class"""
    one = _batch(synthetic.mutag_shaped(24), min_rows_per_class=1)
    b = _batch(synthetic.mutag_shaped(24).replicate(4))
    assert b.LAYER2_MIN_ROWS_PER_CLASS == 8 and _eligible(b)
    assert _check_index(b) == (one.layer2_table_index()[1].numel() - 1) // 4


def test_golden_graphs_agree_with_the_brute_force_eligibility():
    """the golden set has triangles and rows of more than 8 sources: refused, as the four conditions say; its triangle-free
    graphs of small degree are indexed"""
    b = _batch(golden_graphs(), min_rows_per_class=1)
    assert not _eligible(b) and b.layer2_table_index() is None
    sub = []
    for g in golden_graphs():
        s = _batch([g], min_rows_per_class=1)
        if _eligible(s):
            sub.append(g)
        else:
            assert s.layer2_table_index() is None
    if sub:
        _check_index(_batch(sub, min_rows_per_class=1))


@pytest.mark.parametrize("name", ["syn8", "one_neighborhood", "triangle"])
def test_layer2_index_refusals(name):
    if name == "syn8":                                   # refused on degree, before any sort
        b = _batch(synthetic.syn_1827_shaped(8))
        vr = np.asarray(b.part.vrowptr, dtype=np.int64)
        assert (vr[4:4 * b.num_count + 1:4] - vr[0:4 * b.num_count:4]).max() > 8
        assert b.layer2_table_index() is None and "_degree_table" not in b.__dict__
    elif name == "one_neighborhood":                     # 8 U_2 > num_count
        b = _batch([_path(2)])
        assert b.num_graphs == 1
        assert b.layer2_table_index() is None
        b = _batch(synthetic.mutag_shaped(24))
        assert not _eligible(b) and b.layer2_table_index() is None
    else:                                                # a triangle: no empty table slot, no narrow canonical table
        b = _batch([_ring(6), _path(6), TRIANGLE] * 20, min_rows_per_class=1)
        assert b.table_empty == 0 and b.layer2_table_index() is None


def test_new_entry_points_validate_their_arguments():
    """fake aligned host pointers, never dereferenced: every call is refused before any HIP call"""
    L = _lib.lib()
    buf = np.zeros(64 * 1024, np.float32)
    idx = np.zeros(64, np.int32)
    p, q = buf.ctypes.data, idx.ctypes.data
    o, part = p + 65536, p + 131072

    def rows(table=p, ldt=64, nt=4, cls=q, n=16, out=o, ldo=64, bits=q, slot=q, part=part):
        return L.desco_table_rows_pool_f32(table, ldt, nt, cls, n, out, ldo, bits, slot, part, None)

    for kw in (dict(table=None), dict(cls=None), dict(bits=None), dict(slot=None), dict(part=None), dict(n=-1), dict(nt=0),
               dict(nt=2 ** 31), dict(ldt=32), dict(ldt=66), dict(table=p + 4), dict(out=o + 4), dict(ldo=66),
               dict(part=part + 4), dict(out=p)):
        assert L.desco_rng_next(None, None, None) == -1          # (another entry point's message in between)
        assert rows(**kw) == -1, kw
        assert b"desco_table_rows_pool_f32" in L.desco_last_error(), (kw, L.desco_last_error())
    assert rows(n=0) == 0                                        # nothing to do: no launch
    for args in ((None, 4, 4, q), (q, 4, 4, None), (q, -1, 4, q), (q, 4, -1, q)):
        assert L.desco_index_range_check_i32(*args, None) == -1
        assert b"desco_index_range_check_i32" in L.desco_last_error()
    assert L.desco_index_range_check_i32(q, 0, 4, q, None) == 0
