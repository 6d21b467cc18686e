"""Exact per-edge orbit counts (edge graphlet degree vectors) on the host: ``groundtruth.edge_orbit_counts(backend="host")``
against the brute-force yardstick tests/edge_orbit_reference.py, the identities the definition implies (the tie to the
node orbit counts among them), the table, the Python surface's refusals, the Workload cache and the driver's CSV.
No GPU."""
import ctypes
import itertools

import networkx as nx
import numpy as np
import pytest
import torch

import edge_orbit_reference as R
from desco_amd.graphs import GraphSet
from desco_amd.groundtruth import (canonical_counts, census_classes, edge_orbit_columns, edge_orbit_counts,
                                   edge_orbit_noninduced_matrix, edge_orbit_rows, orbit_columns, orbit_counts)
from helpers import golden_graphs, random_family_graphs

CENSUS = [q for k in (2, 3, 4, 5) for q in census_classes(k)]
COLS = edge_orbit_columns()
FORMS = [True, False]
P3, TRIANGLE = (3, [(0, 1), (1, 2)]), (3, [(0, 1), (1, 2), (0, 2)])


def host(graphs, queries=None, induced=True, **kw):
    gs = graphs if isinstance(graphs, GraphSet) else GraphSet.from_edge_lists(graphs)
    return edge_orbit_counts(gs, queries, backend="host", induced=induced, **kw)


def edges_of(g):
    return (g.number_of_nodes(), [tuple(e) for e in g.edges()])


def shuffled(graph, rng):
    n, edges = graph
    p = rng.permutation(n)
    return (n, [(int(p[a]), int(p[b])) for a, b in edges])


@pytest.fixture(scope="module")
def small_graphs():
    rng = np.random.default_rng(17)
    out = [edges_of(nx.path_graph(7)), edges_of(nx.cycle_graph(8)), edges_of(nx.star_graph(7)),
           edges_of(nx.wheel_graph(7)), edges_of(nx.complete_graph(5)), edges_of(nx.complete_graph(6)),
           edges_of(nx.petersen_graph()),
           (0, []), (1, []), (2, [(0, 1)]), (9, [(0, 5), (5, 7), (7, 0), (7, 8), (2, 8)])]   # empty graph .. isolated nodes
    out += [shuffled(edges_of(nx.gnp_random_graph(int(rng.integers(6, 13)), float(rng.uniform(0.2, 0.55)), seed=300 + i)),
                     rng) for i in range(4)]
    return out


@pytest.fixture(scope="module")
def family():
    gs = GraphSet.from_edge_lists(random_family_graphs(43, 60))
    return gs, {f: host(gs, induced=f) for f in FORMS}


def incidence(gs):
    """[N, M] doubles: 1 where the node is an end of the edge"""
    ends = edge_orbit_rows(gs)
    b = torch.zeros((gs.num_nodes, ends.shape[0]), dtype=torch.double)
    b[ends[:, 0], torch.arange(ends.shape[0])] = 1
    b[ends[:, 1], torch.arange(ends.shape[0])] = 1
    return b


# ---- the yardstick itself, on closed forms, before it is used --------------------------------------------------------
def test_yardstick_on_closed_forms():
    diamond = (4, [(0, 1), (1, 2), (2, 3), (3, 0), (0, 2)])
    tailed = (4, [(0, 1), (1, 2), (0, 2), (2, 3)])
    assert R.edge_orbits(P3)[1] == [((0, 1), (1, 2))] and R.edge_orbits(TRIANGLE)[1] == [((0, 1), (0, 2), (1, 2))]
    assert R.edge_orbits(diamond)[1] == [((0, 1), (1, 2), (0, 3), (2, 3)), ((0, 2),)]         # the rim, the chord
    assert R.edge_orbits(tailed)[1] == [((0, 1),), ((0, 2), (1, 2)), ((2, 3),)]               # opposite, at the joint, tail
    assert len(R.columns(CENSUS)) == 69
    k4 = edges_of(nx.complete_graph(4))
    assert R.rows([k4, (2, [(1, 0)])]) == [(0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3), (4, 5)]
    got = R.edge_orbit_counts_reference([k4], [(2, [(0, 1)]), P3, TRIANGLE, diamond])
    assert (got == np.array([[1, 0, 2, 0, 0]] * 6)).all()
    got = R.edge_orbit_counts_reference([k4], [(2, [(0, 1)]), P3, TRIANGLE, diamond], induced=False)
    assert (got == np.array([[1, 4, 2, 4, 1]] * 6)).all()                 # 6 diamonds in K4: rim of 4, chord of 1
    star = (5, [(0, i) for i in range(1, 5)])
    assert (R.edge_orbit_counts_reference([star], [P3, (4, [(0, 1), (0, 2), (0, 3)])]) == [[3, 3]] * 4).all()


# ---- columns, rows, table --------------------------------------------------------------------------------------------
def test_columns_of_the_census():
    assert len(COLS) == 69
    assert [sum(1 for qi, _, _ in COLS if CENSUS[qi][0] == k) for k in (2, 3, 4, 5)] == [1, 2, 10, 56]
    for qi, (k, edges) in enumerate(CENSUS):
        mine = [(o, mem) for q, o, mem in COLS if q == qi]
        assert [o for o, _ in mine] == list(range(len(mine)))
        assert sorted(e for _, mem in mine for e in mem) == sorted((min(a, b), max(a, b)) for a, b in edges)
        firsts = [R.rank(mem[0]) for _, mem in mine]
        assert firsts == sorted(firsts)                                      # ascending smallest member
    assert COLS == R.columns(CENSUS)


def test_rows_follow_the_csr(small_graphs):
    gs = GraphSet.from_edge_lists(small_graphs)
    rows = edge_orbit_rows(gs)
    assert rows.dtype == torch.int64 and rows.tolist() == [list(e) for e in R.rows(small_graphs)]
    assert edge_orbit_rows(GraphSet.from_edge_lists([])).shape == (0, 2)


def c_table(queries):
    from desco_amd import _lib
    from desco_amd.groundtruth import _flatten_queries
    L = _lib.lib()
    table = np.full((1098, 10), 77, np.int16)
    ncol, kmax = ctypes.c_int(0), ctypes.c_int(0)
    _, qn, qp, qe = _flatten_queries(queries)
    rc = L.desco_edge_orbit_table(qn.ctypes.data, qp.ctypes.data, qe.ctypes.data if len(qe) else None, len(qn),
                                  table.ctypes.data, ctypes.byref(ncol), ctypes.byref(kmax))
    return rc, table, ncol.value, kmax.value, L.desco_last_error()


def test_table_rows_are_consistent_with_the_mask_class():
    rc, table, ncol, kmax, _ = c_table(CENSUS)
    assert rc == 0 and (ncol, kmax) == (69, 5)
    owner = [qi for qi, _, _ in COLS]
    sizes = [len(mem) for _, _, mem in COLS]
    graphs = [nx.Graph() for _ in CENSUS]
    for g, (k, edges) in zip(graphs, CENSUS):
        g.add_nodes_from(range(k))
        g.add_edges_from(edges)
    off = {2: 0, 3: 2, 4: 10, 5: 74}
    connected_masks = 0
    for k in (2, 3, 4, 5):
        pairs = [(a, b) for b in range(1, k) for a in range(b)]              # in pair-bit order
        for mask in range(1 << len(pairs)):
            row = table[off[k] + mask]
            h = nx.Graph()
            h.add_nodes_from(range(k))
            h.add_edges_from(p for i, p in enumerate(pairs) if mask >> i & 1)
            if not nx.is_connected(h):
                assert (row == -1).all()
                continue
            connected_masks += 1
            assert all((row[i] >= 0) == bool(mask >> i & 1) for i in range(len(pairs))) and (row[len(pairs):] == -1).all()
            used = [int(c) for c in row if c >= 0]
            qi = owner[used[0]]
            assert all(owner[c] == qi for c in used) and nx.is_isomorphic(h, graphs[qi])
            assert all(used.count(c) == sizes[c] for c in set(used))         # every orbit in full
            assert sorted(set(used)) == [j for j, q in enumerate(owner) if q == qi]
    assert connected_masks == 1 + 4 + 38 + 728
    rc, table, ncol, kmax, _ = c_table([P3])
    assert rc == 0 and (ncol, kmax) == (1, 3) and (table[:2] == -1).all() and (table[10:] == -1).all()
    assert table[2 + 0b011].tolist() == [0, 0] + [-1] * 8 and table[2 + 0b110].tolist() == [-1, 0, 0] + [-1] * 7
    assert (table[2 + 0b111] == -1).all()                                    # the triangle was not asked for


# ---- against the yardstick -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("induced", FORMS)
def test_host_equals_the_yardstick(small_graphs, induced):
    got = host(small_graphs, induced=induced)
    assert got.dtype == torch.double and got.shape == (sum(len(set(map(frozenset, e))) for _, e in small_graphs), 69)
    ref = R.edge_orbit_counts_reference(small_graphs, CENSUS, induced=induced)
    assert ref.sum() > 0
    assert (got.numpy() == ref).all()


# ---- identities on graphs too big for the yardstick ------------------------------------------------------------------
@pytest.mark.parametrize("induced", FORMS)
def test_column_sums_are_orbit_size_times_canonical(family, induced):
    gs, eorb = family
    canon = canonical_counts(gs, CENSUS, backend="host", induced=induced)
    node_graph = torch.from_numpy(gs.node_graph_ids()).long()
    edge_graph = node_graph[edge_orbit_rows(gs)[:, 1]]
    per_graph = lambda t, gid: torch.zeros((gs.num_graphs, t.shape[1]), dtype=t.dtype).index_add_(0, gid, t)   # noqa: E731
    o, c = per_graph(eorb[induced], edge_graph), per_graph(canon, node_graph)
    for j, (qi, _, mem) in enumerate(COLS):
        assert (o[:, j] == len(mem) * c[:, qi]).all(), (j, qi)
    assert o.sum() > 0


@pytest.mark.parametrize("induced", FORMS)
def test_closed_form_columns(family, induced):
    gs, eorb = family
    e = eorb[induced]
    ends = edge_orbit_rows(gs)
    deg = torch.from_numpy(np.diff(gs.rowptr)).double()
    adj = torch.zeros((gs.num_nodes, gs.num_nodes), dtype=torch.double)
    adj[ends[:, 0], ends[:, 1]] = adj[ends[:, 1], ends[:, 0]] = 1
    common = (adj[ends[:, 0]] * adj[ends[:, 1]]).sum(1)
    edge, p3, tri = (R.column_of(CENSUS, q, (0, 1)) for q in ((2, [(0, 1)]), P3, TRIANGLE))
    assert (edge, p3, tri) == (0, 1, 2)
    assert (e[:, edge] == 1).all()
    assert (e[:, tri] == common).all() and common.sum() > 0
    wedge = deg[ends[:, 0]] + deg[ends[:, 1]] - 2
    assert (e[:, p3] == (wedge - 2 * common if induced else wedge)).all()


@pytest.mark.parametrize("induced", FORMS)
def test_tie_to_the_node_orbit_counts(family, induced):
    """sum over the edges at v of eorb[e][(q,o)] = sum_p orbit[v][(q,p)] * inc_q[p][o], inc_q[p][o] = the edges of
    orbit o at a node of node orbit p of q"""
    gs, eorb = family
    node = orbit_counts(gs, backend="host", induced=induced)
    ncols = orbit_columns()
    inc = torch.zeros((len(ncols), len(COLS)), dtype=torch.double)
    for i, (qi, _, positions) in enumerate(ncols):
        for j, (qj, _, members) in enumerate(COLS):
            if qi == qj:
                inc[i, j] = sum(1 for edge in members if positions[0] in edge)
    weight = torch.tensor([len(positions) for _, _, positions in ncols], dtype=torch.double)
    assert (weight @ inc).tolist() == [2.0 * len(members) for _, _, members in COLS]    # every edge has two ends
    lhs, rhs = incidence(gs) @ eorb[induced], node @ inc
    assert torch.equal(lhs, rhs) and lhs.sum() > 0


@pytest.mark.parametrize("induced", FORMS)
def test_relabelling_permutes_the_rows(family, induced):
    gs, eorb = family
    rng = np.random.default_rng(5)
    graphs, perm, base = [], [], 0
    for n, edges in gs.edge_lists():
        p = rng.permutation(n)
        graphs.append((n, [(int(p[a]), int(p[b])) for a, b in edges]))
        perm += [base + int(p[v]) for v in range(n)]
        base += n
    gs2 = GraphSet.from_edge_lists(graphs)
    got = host(gs2, induced=induced)
    row_of = {tuple(e): i for i, e in enumerate(edge_orbit_rows(gs2).tolist())}
    rows = [row_of[tuple(sorted((perm[u], perm[v])))] for u, v in edge_orbit_rows(gs).tolist()]
    assert sorted(rows) == list(range(len(rows))) and rows != sorted(rows)
    assert (got[rows] == eorb[induced]).all()


@pytest.mark.parametrize("induced", FORMS)
def test_per_query_sums(family, induced):
    gs, eorb = family
    pq = host(gs, induced=induced, per_query=True)
    assert pq.shape == (eorb[induced].shape[0], 30)
    for qi in range(30):
        assert (pq[:, qi] == eorb[induced][:, [j for j, c in enumerate(COLS) if c[0] == qi]].sum(1)).all()
    k, edges = CENSUS[2]
    assert len(edges) == 3 and (pq[:, 2] == eorb[induced][:, 2]).all()     # triangles through the edge: its support


def test_thread_count_does_not_change_the_result(family):
    gs, eorb = family
    for induced in FORMS:
        assert torch.equal(host(gs, induced=induced, num_threads=1), host(gs, induced=induced, num_threads=4))
        assert torch.equal(host(gs, induced=induced, num_threads=4), eorb[induced])


# ---- the queries' own positions --------------------------------------------------------------------------------------
@pytest.mark.parametrize("induced", FORMS)
def test_duplicate_isomorphic_and_reordered_queries(small_graphs, induced):
    tailed_a = (4, [(0, 1), (1, 2), (0, 2), (2, 3)])                         # tail 2-3
    tailed_b = (4, [(3, 1), (1, 2), (3, 2), (1, 0)])                         # the same class: tail 0-1
    p4 = nx.Graph([("x", "y"), ("y", "z"), ("z", "w")])                     # positions x, y, z, w: middle edge 1-2
    p4_b = (4, [(0, 2), (2, 3), (3, 1)])                                     # middle edge 2-3
    queries = [tailed_a, tailed_b, p4, tailed_a, p4_b, TRIANGLE]
    cols = edge_orbit_columns(queries)
    assert cols == R.columns(queries)
    assert [mem for qi, _, mem in cols if qi == 1] == [((0, 1),), ((1, 2), (1, 3)), ((2, 3),)]
    assert [mem for qi, _, mem in cols if qi == 4] == [((0, 2), (1, 3)), ((2, 3),)]
    graphs = small_graphs[3:]
    got = host(graphs, queries, induced=induced)
    assert (got.numpy() == R.edge_orbit_counts_reference(graphs, queries, induced=induced)).all()
    assert got.sum() > 0 and torch.equal(got[:, 0:3], got[:, 8:11])
    full = host(graphs, induced=induced)                                     # reordered census classes
    order = [20, 0, 5, 29, 12, 1]
    pick = [j for qi in order for j, c in enumerate(COLS) if c[0] == qi]
    assert torch.equal(host(graphs, [CENSUS[i] for i in order], induced=induced), full[:, pick])


def test_transform_matrix():
    t3 = edge_orbit_noninduced_matrix(3)             # columns: the P3 edge, the triangle edge
    assert t3.dtype == np.int64 and t3.tolist() == [[1, 0], [2, 1]]         # a triangle's edge lies in two of its P3s
    assert edge_orbit_noninduced_matrix(3) is t3     # cached
    for k in (2, 3, 4, 5):
        t = edge_orbit_noninduced_matrix(k)
        classes = list(census_classes(k))
        assert t.shape[0] == t.shape[1] == [1, 2, 10, 56][k - 2] and (np.diag(t) == 1).all() and (t >= 0).all()
        # against the brute force on the class representatives: the row of an edge of c is T's row of its orbit
        ref = R.edge_orbit_counts_reference(classes, classes, induced=False)
        row, r0 = 0, 0
        for c in classes:
            orbit_of = R.edge_orbits(c)[0]
            n_orb = max(orbit_of.values()) + 1
            for u, v in R.rows([c]):
                assert (ref[row] == t[r0 + orbit_of[(u, v)]]).all(), (k, c, (u, v))
                row += 1
            r0 += n_orb
        assert row == ref.shape[0] and r0 == t.shape[0]


# ---- refusals, empty input -------------------------------------------------------------------------------------------
def test_refusals_and_empty_inputs():
    gs = GraphSet.from_edge_lists([(4, [(0, 1), (1, 2)])])
    with pytest.raises(RuntimeError, match=r"edge orbit counts take queries of 2\.\.5 nodes"):
        host(gs, [(6, [(i, i + 1) for i in range(5)])])
    with pytest.raises(RuntimeError, match=r"edge orbit counts take queries of 2\.\.5 nodes"):
        edge_orbit_columns([nx.path_graph(7)])
    with pytest.raises(RuntimeError) as disconnected:
        host(gs, [(4, [(0, 1), (2, 3)])])
    with pytest.raises(RuntimeError) as looped:
        host(gs, [(3, [(0, 1), (1, 2), (2, 2)])])
    from desco_amd.groundtruth import match_plan
    for err, q in ((disconnected, (4, [(0, 1), (2, 3)])), (looped, (3, [(0, 1), (1, 2), (2, 2)]))):
        with pytest.raises(RuntimeError) as plan:
            match_plan([q])
        assert str(err.value) == str(plan.value)                           # the matcher plan's message
    with pytest.raises(ValueError, match="unknown backend"):
        edge_orbit_counts(gs, backend="vf2")
    assert host(gs, []).shape == (2, 0) and host(gs, [], per_query=True).shape == (2, 0)
    assert host(GraphSet.from_edge_lists([])).shape == (0, 69)
    assert host(GraphSet.from_edge_lists([(3, [])]), induced=False).shape == (0, 69)


def test_c_level_refusals_name_the_limit():
    """desco_edge_orbit_table, desco_edge_orbit_counts and desco_edge_orbit_counts_dev refuse what they do not take with
    DESCO_EINVAL and a message naming the entry point and the limit -- the device entry before any HIP call"""
    from desco_amd import _lib
    L = _lib.lib()
    for queries, word in (([(6, [(i, i + 1) for i in range(5)])], b"2..5 nodes"),
                          ([(1, [])], b"2..5 nodes"),
                          ([(4, [(0, 1), (2, 3)])], b"connected"),
                          ([(3, [(0, 1), (1, 3)])], b"bad query edge"),
                          ([P3, (3, [(0, 2), (2, 1)])], b"isomorphic")):
        rc, _, _, _, err = c_table(queries)
        assert rc == -1 and word in err and b"desco_edge_orbit_table" in err
    assert L.desco_edge_orbit_table(None, None, None, 1, None, None, None) == -1
    assert b"desco_edge_orbit_table: bad argument" in L.desco_last_error()
    gs = GraphSet.from_edge_lists([(3, [(0, 1), (1, 2)])])
    out = np.zeros((2, 69), np.int64)
    qn, qp, qe = np.array([6], np.int32), np.array([0, 1], np.int32), np.array([0, 1], np.int32)
    assert L.desco_edge_orbit_counts(gs.graph_ptr.ctypes.data, 1, gs.rowptr.ctypes.data, gs.col.ctypes.data,
                                     qn.ctypes.data, qp.ctypes.data, qe.ctypes.data, 1, 1, out.ctypes.data) == -1
    assert b"2..5 nodes" in L.desco_last_error()
    assert L.desco_edge_orbit_counts(None, 1, None, None, None, None, None, 1, 1, None) == -1
    assert b"desco_edge_orbit_counts: bad argument" in L.desco_last_error()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data                              # host memory: a refused call never touches it

    def dev(table=p, kmax=5, columns=69, entry_row=p, rows=1, entries=2, col=p):
        return L.desco_edge_orbit_counts_dev(p, 1, 4, p, entries, col, p, p, p, 1, entry_row, rows, table, kmax, columns,
                                             p, None)

    for bad in (dict(columns=70), dict(table=None), dict(kmax=6), dict(kmax=1), dict(entry_row=None), dict(col=None),
                dict(rows=3), dict(entries=2 ** 31)):
        assert L.desco_gemm_f32_multi(5, None, None) == -1                   # (another entry point's message in between)
        assert dev(**bad) == -1 and b"desco_edge_orbit_counts_dev" in L.desco_last_error(), bad
    assert dev(rows=0) == 0 and dev(columns=0) == 0 and dev(entries=0, rows=0) == 0          # nothing to do
    assert (buf == 0).all()


# ---- Workload and the driver -----------------------------------------------------------------------------------------
def test_workload_cache_round_trip(tmp_path):
    from desco_amd.workload import Workload
    graphs = golden_graphs(max_n=14)[:6]
    edges = sum(len(e) for _, e in GraphSet.from_edge_lists(graphs).edge_lists())
    w = Workload(GraphSet.from_edge_lists(graphs), str(tmp_path))
    assert w.edge_orbit_count_truth is None and not w.exist_edge_orbit_groundtruth()
    truth = w.compute_edge_orbit_groundtruth()
    assert truth is w.edge_orbit_count_truth and truth.shape == (edges, 69)
    non = w.compute_edge_orbit_groundtruth(induced=False)
    tri = [TRIANGLE, P3]
    w.compute_edge_orbit_groundtruth(queries=tri)
    w.compute_edge_orbit_groundtruth(induced=False, save_to_file=False, queries=[tri[0]])
    folder = tmp_path / "EdgeOrbitCountTruth"
    assert sorted(p.name for p in folder.iterdir()) == [
        "edge_orbit_columns_2_query_num_2_query_len_sum_6.pt",
        "edge_orbit_columns_69_query_num_30_query_len_sum_137.pt",
        "edge_orbit_columns_69_query_num_30_query_len_sum_137_noninduced.pt"]
    w2 = Workload(GraphSet.from_edge_lists(graphs), str(tmp_path))
    assert w2.exist_edge_orbit_groundtruth() and w2.exist_edge_orbit_groundtruth(induced=False)
    assert w2.exist_edge_orbit_groundtruth(queries=tri) and not w2.exist_edge_orbit_groundtruth(queries=tri, induced=False)
    assert torch.equal(w2.load_edge_orbit_groundtruth(), truth) and w2.edge_orbit_count_truth is not None
    assert torch.equal(w2.load_edge_orbit_groundtruth(induced=False), non) and not torch.equal(non, truth)
    assert not (tmp_path / "CanonicalCountTruth").exists() and not (tmp_path / "OrbitCountTruth").exists()


def test_workload_refuses_node_features(tmp_path):
    from desco_amd.workload import Workload
    gs = GraphSet.from_edge_lists([(3, [(0, 1), (1, 2)])])
    gs.node_feat = np.eye(3, dtype=np.float32)
    w = Workload(gs, str(tmp_path), node_feat_len=3)
    with pytest.raises(NotImplementedError, match="labelled"):
        w.compute_edge_orbit_groundtruth()


def test_driver_flag_and_csv(tmp_path):
    """``main.py --edge_orbit_truth`` travels on args_opt and leaves no trace when absent; the table it writes for a toy
    test set holds the two endpoint columns, then the 69 count columns under their (query, orbit) header"""
    import pandas as pd
    import main as driver
    from desco_amd.workload import Workload
    args, _, _, args_opt = driver.parse_args([])
    assert not hasattr(args, "edge_orbit_truth") and not hasattr(args_opt, "edge_orbit_truth")
    args, _, _, args_opt = driver.parse_args(["--edge_orbit_truth"])
    assert args.edge_orbit_truth is True and args_opt.edge_orbit_truth is True and not hasattr(args_opt, "orbit_truth")
    from desco_amd import config
    assert "edge_orbit_truth" not in open(config.__file__).read()
    graphs = [edges_of(nx.complete_graph(4)), (3, [(2, 0)]), edges_of(nx.cycle_graph(5))]
    out = tmp_path / "out"
    out.mkdir()
    w = Workload(GraphSet.from_edge_lists(graphs), str(tmp_path / "toy"))
    for _ in range(2):                               # computed, then loaded from the cache
        path = driver.write_edge_orbit_truth(w, str(out), "toy")
        assert path == str(out / "orbit_edge_toy.csv") and w.exist_edge_orbit_groundtruth()
        table = pd.read_csv(path, index_col=0)
        assert list(table.columns) == ["u", "v"] + [f"({q},{o})" for q, o, _ in COLS] and table.shape == (12, 71)
        assert table[["u", "v"]].to_numpy().tolist() == [list(e) for e in R.rows(graphs)]
        assert (table.to_numpy()[:, 2:] == R.edge_orbit_counts_reference(graphs, CENSUS)).all()
    path = driver.write_edge_orbit_truth(w, str(out), "toy", induced=False)
    assert (pd.read_csv(path, index_col=0).to_numpy()[:, 2:] ==
            R.edge_orbit_counts_reference(graphs, CENSUS, induced=False)).all()
