"""Host side of gnn_model.ANCHOR_CLASS_TABLE: NeighborhoodBatch.anchor_class_index on CPU tensors against a brute-force dict
over the tuples that define the classes -- a canonical row of X_L by (its canonical class of X_{L-1}, the count classes of
X_{L-1} of its ordered sources), level by level from the first-layer tables up, as tests/test_deep_tables_host.py does for the
levels below.

The partitions are degree-sorted, as InferencePipeline's are.  The small blocks lower the profit bounds on their own batch
object; the defaults are tested as refusals."""
import numpy as np
import pytest

from desco_amd import synthetic
from desco_amd.batch import NeighborhoodBatch
from desco_amd.graphs import GraphSet
from desco_amd.partition import build_partition

S = 4


def _batch(graphs, min_rows=1, per_class=1, max_level=None):
    gs = graphs if isinstance(graphs, GraphSet) else GraphSet.from_edge_lists(graphs)
    b = NeighborhoodBatch(build_partition(gs, 4).degree_sorted(), "cpu")
    b.LAYER3_MIN_ROWS, b.LAYER3_MIN_ROWS_PER_CLASS, b.LAYER2_MIN_ROWS_PER_CLASS = 1, 1, 1
    b.DEEP_TABLE_MIN_ROWS, b.DEEP_TABLE_MIN_ROWS_PER_CLASS, b.DEEP_TABLE_MAX_CLASSES = 1, 1, 1 << 17
    if min_rows is not None:
        b.ANCHOR_CLASS_MIN_ROWS = min_rows
    if per_class is not None:
        b.ANCHOR_CLASS_MIN_ROWS_PER_CLASS = per_class
    if max_level is not None:
        b.DEEP_TABLE_MAX_LEVEL = max_level
    return b


def _brute_force(b, top=8):
    """{level j: (count classes [num_count], canonical classes [B])} for j = 1 .. top, the ids numbered by first appearance"""
    nc, n = b.num_count, b.num_rows
    vr = np.asarray(b.part.vrowptr, dtype=np.int64).tolist()
    vcol = np.asarray(b.part.vcol, dtype=np.int64).tolist()
    cls = b.degree_table_index()[1].tolist()
    ccls = b.canonical_table_index()[1].tolist()
    out = {1: (cls, ccls)}
    for j in range(1, top):
        cd, nd = {}, {}
        ccls_n = [cd.setdefault((ccls[q], tuple(cls[s] for s in vcol[vr[S * (nc + q)]:vr[S * (nc + q) + S]])), len(cd))
                  for q in range(n - nc)]
        cls_n = [nd.setdefault((cls[i], tuple(cls[s] for s in vcol[vr[S * i]:vr[S * i + 2]]),
                                tuple(ccls[s - nc] for s in vcol[vr[S * i + 2]:vr[S * i + S]])), len(nd)) for i in range(nc)]
        cls, ccls = cls_n, ccls_n
        out[j + 1] = (cls, ccls)
    return out


def _same_partition(a, b):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    return a.shape == b.shape and len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))


def _refines(fine, coarse):
    """every class of ``fine`` lies inside one class of ``coarse``"""
    return len(set(zip(np.asarray(fine).tolist(), np.asarray(coarse).tolist()))) == len(set(np.asarray(fine).tolist()))


def _small_set():
    """hand-made molecule-like graphs without triangles: rings, paths, a star, a branched ring"""
    ring = lambda k: (k, [(i, (i + 1) % k) for i in range(k)])
    path = lambda k: (k, [(i, i + 1) for i in range(k - 1)])
    star = (5, [(0, i) for i in range(1, 5)])
    branched = (9, [(i, (i + 1) % 6) for i in range(6)] + [(0, 6), (6, 7), (3, 8)])
    return [ring(6), path(6), star, branched, ring(5), path(9), ring(8), branched] * 3


SETS = {"mutag24": lambda: synthetic.mutag_shaped(24), "cox2_12": lambda: synthetic.cox2_shaped(12), "small": _small_set}


@pytest.fixture(scope="module")
def built():
    """per set: the batch at L = 8 with its brute-force classes (computed once, left unchanged)"""
    out = {}
    for name, make in SETS.items():
        b = _batch(make())
        out[name] = (b, _brute_force(b))
    return out


@pytest.mark.parametrize("name", list(SETS))
def test_the_classes_are_the_dictionarys_and_the_representatives_their_lowest_rows(built, name):
    b, bf = built[name]
    nc, n = b.num_count, b.num_rows
    assert len(b.deep_table_index()) == 5
    idx = b.anchor_class_index(8)
    assert idx is not None and b.anchor_class_index(8) is idx                      # built once, cached
    acls, arep = idx
    assert acls.dtype.is_floating_point is False and acls.element_size() == 4 and arep.element_size() == 8
    acls, arep = acls.numpy().astype(np.int64), arep.numpy()
    ua = len(set(bf[8][1]))
    # ids dense, the class count and the classes the brute force's
    assert acls.shape == (n - nc,) and sorted(set(acls.tolist())) == list(range(ua)) and _same_partition(acls, bf[8][1])
    # each representative is its class's lowest row
    first = {}
    for q, c in enumerate(acls.tolist()):
        first.setdefault(c, q)
    assert arep.shape == (ua,) and [first[c] for c in range(ua)] == arep.tolist()
    # nested level to level: the classes of X_8 refine those of X_7 .. X_1 (the index's own and the dictionary's), so one
    # class agrees in the canonical rows of every layer
    assert _refines(acls, b.canonical_table_index()[1].numpy())
    for k in range(3, 9):
        assert _refines(acls, b._table_level(k)[5].numpy()), k
    for j in range(1, 8):
        assert _refines(acls, bf[j][1]) and _refines(bf[j + 1][1], bf[j][1]), j


@pytest.mark.parametrize("name", ["mutag24", "small"])
@pytest.mark.parametrize("L", [4, 5])
def test_a_shallower_model_takes_the_level_that_is_its_last(built, name, L):
    b = _batch(SETS[name](), max_level=L)
    assert len(b.deep_table_index()) == L - 3
    acls, arep = b.anchor_class_index(L)
    bf = built[name][1]
    assert _same_partition(acls.numpy(), bf[L][1]) and arep.numel() == len(set(bf[L][1]))
    # ... and is the next level's canonical classes where the deeper index exists
    assert _same_partition(acls.numpy(), built[name][0]._table_level(L + 1)[5].numpy())


def test_replication_adds_no_class():
    one = _batch(synthetic.mutag_shaped(24))
    four = _batch(synthetic.mutag_shaped(24).replicate(4))
    assert four.num_rows - four.num_count == 4 * (one.num_rows - one.num_count)
    assert four.anchor_class_index(8)[1].numel() == one.anchor_class_index(8)[1].numel()


@pytest.mark.parametrize("name", ["levels", "rows", "rows_per_class", "dense", "no deep tables"])
def test_refusals(name):
    g = synthetic.mutag_shaped(24)
    ua = _batch(g).anchor_class_index(8)[1].numel()
    if name == "levels":                                 # K < L, K > L, models without a deep level
        b = _batch(g, max_level=6)
        assert len(b.deep_table_index()) == 3
        assert b.anchor_class_index(8) is None and b.anchor_class_index(7) is None and b.anchor_class_index(5) is None
        assert b.anchor_class_index(3) is None and b.anchor_class_index(2) is None
        assert b.anchor_class_index(6) is not None
    elif name == "rows":                                 # below ANCHOR_CLASS_MIN_ROWS neighborhoods: refused before any work
        b = _batch(g.replicate(2), min_rows=None)
        B = b.num_rows - b.num_count
        assert b.ANCHOR_CLASS_MIN_ROWS == NeighborhoodBatch.ANCHOR_CLASS_MIN_ROWS >= 1 << 20 > B
        assert b.anchor_class_index(8) is None and "_deep_table" not in b.__dict__
        b = _batch(g.replicate(2), min_rows=B + 1)
        assert b.anchor_class_index(8) is None
        b = _batch(g.replicate(2), min_rows=B)
        assert b.anchor_class_index(8) is not None
    elif name == "rows_per_class":                       # ANCHOR_CLASS_MIN_ROWS_PER_CLASS U_a > B, at the bound and one past
        b = _batch(g, per_class=None)
        B = b.num_rows - b.num_count
        assert b.ANCHOR_CLASS_MIN_ROWS_PER_CLASS == NeighborhoodBatch.ANCHOR_CLASS_MIN_ROWS_PER_CLASS == 8 and 8 * ua > B
        assert b.anchor_class_index(8) is None
        r = _batch(g.replicate(2), per_class=2 * B // ua)
        assert r.anchor_class_index(8) is not None
        r = _batch(g.replicate(2), per_class=2 * B // ua + 1)
        assert r.anchor_class_index(8) is None
    elif name == "dense":                                # rows of degree above 8: no table level at all
        b = _batch(synthetic.syn_1827_shaped(8))
        assert b.deep_table_index() == [] and b.anchor_class_index(8) is None
    else:                                                # the deep tables' own bounds refuse: nothing to build on
        b = _batch(g)
        b.DEEP_TABLE_MIN_ROWS = b.num_count + 1
        assert b.deep_table_index() == [] and b.anchor_class_index(8) is None


def test_a_canonical_row_of_degree_above_eight_refuses():
    # a star of nine leaves: its centre's canonical row has nine sources (and so has the centre's count row: no level at all)
    star = (10, [(0, i) for i in range(1, 10)])
    b = _batch([star, (6, [(i, i + 1) for i in range(5)])] * 30)
    assert b._level_csr() is None and b.anchor_class_index(8) is None
    # the canonical rows' own bound, alone: the block's CSR summary with a longest canonical segment of nine
    b = _batch(synthetic.mutag_shaped(24))
    c = b._level_csr()
    assert c.cdmax <= b.LAYER2_MAX_DEGREE
    b._level_csr = lambda: c._replace(cdmax=b.LAYER2_MAX_DEGREE + 1)
    assert b.layer2_table_index() is not None and b.layer3_table_index() is None and b.anchor_class_index(8) is None


@pytest.mark.parametrize("L", [8, 5])
@pytest.mark.parametrize("name", list(SETS))
def test_the_canonical_tables_of_every_level(built, name, L):
    """canonical_class_tables: per level the compact CSR of the classes' lowest rows with the sources as count classes of the
    level below, the representatives' own classes below, the rows of the anchor operand's blocks -- against the block's CSR
    and the classes of the dictionary"""
    b = built[name][0] if L == 8 else _batch(SETS[name](), max_level=L)
    bf = built[name][1]
    nc, n = b.num_count, b.num_rows
    t = b.canonical_class_tables(L)
    assert t is not None and b.canonical_class_tables(L) is t                      # built once, cached
    acls, arep = (x.numpy().astype(np.int64) for x in b.anchor_class_index(L))
    vr = np.asarray(b.part.vrowptr, dtype=np.int64)
    vcol = np.asarray(b.part.vcol, dtype=np.int64)
    # the index's own classes per level: canonical (1 .. L) and count (1 .. L - 1)
    ccls = {1: b.canonical_table_index()[1].numpy().astype(np.int64), L: acls}
    ccls.update({l: b._table_level(l + 1)[5].numpy().astype(np.int64) for l in range(2, L)})
    cls = {1: b.degree_table_index()[1].numpy().astype(np.int64)}
    cls.update({k: b._table_level(k)[0].numpy().astype(np.int64) for k in range(2, L)})
    # class counts: the dictionary's, level by level; the tables side by side in one buffer
    assert list(t.size) == [len(set(bf[l][1])) for l in range(1, L + 1)]
    assert list(t.offset) == [sum(t.size[:l]) for l in range(L)] and len(t.levels) == L - 1
    assert all(_same_partition(ccls[l], bf[l][1]) for l in range(1, L + 1))
    # table 1: the distinct canonical degree tuples
    assert t.uptr1 is b.canonical_table_index()[0] and t.uptr1.numel() == t.size[0] * S + 1
    for l in range(2, L + 1):
        rep_uptr, rep_vcol, below = t.levels[l - 2]
        assert rep_uptr.element_size() == rep_vcol.element_size() == 4 and below.element_size() == 8
        rep_uptr, rep_vcol, below = (x.numpy().astype(np.int64) for x in (rep_uptr, rep_vcol, below))
        uc = t.size[l - 1]
        first = {}
        for q, c in enumerate(ccls[l].tolist()):
            first.setdefault(c, q)
        assert sorted(first) == list(range(uc))
        assert rep_uptr.shape == (uc * S + 1,) and rep_uptr[0] == 0 and rep_vcol.shape == (rep_uptr[-1],) and below.shape == (uc,)
        for c in range(uc):
            r = nc + first[c]                                                     # the class's lowest canonical row
            assert below[c] == ccls[l - 1][first[c]]
            assert np.array_equal(np.diff(rep_uptr[S * c:S * c + S + 1]), np.diff(vr[S * r:S * r + S + 1]))
            seg = vcol[vr[S * r]:vr[S * r + S]]
            assert (seg < nc).all() and rep_vcol[rep_uptr[S * c]:rep_uptr[S * c + S]].tolist() == cls[l - 1][seg].tolist()
        # every id inside its table
        assert rep_vcol.min() >= 0 and rep_vcol.max() <= cls[l - 1].max() and below.min() >= 0 and below.max() < t.size[l - 2]
    rows = t.anchor_rows.numpy().reshape(len(arep), L)
    for l in range(1, L + 1):
        assert np.array_equal(rows[:, l - 1], t.offset[l - 1] + ccls[l][arep])
        assert rows[:, l - 1].min() >= t.offset[l - 1] and rows[:, l - 1].max() < t.offset[l - 1] + t.size[l - 1]


def test_the_canonical_tables_refuse_where_the_anchor_classes_do():
    g = synthetic.mutag_shaped(24)
    assert _batch(g, max_level=6).canonical_class_tables(8) is None
    assert _batch(g, min_rows=None).canonical_class_tables(8) is None
    assert _batch(g, per_class=None).canonical_class_tables(8) is None
    assert _batch(g, max_level=6).canonical_class_tables(6) is not None
