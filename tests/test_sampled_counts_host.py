"""Sampled counts (RAND-ESU) on a CPU-only host: the OpenMP twin (csrc/sampled_counts.cpp) against a pure Python
restatement of the definition (tests/sampled_reference.py), the properties of the decision chain -- exactness at
probability 1, prefix, monotone coupling, slices -- two statistical gates, the estimator, the entry points' argument
checks and the driver."""
import csv
import os
import re
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampled_reference as ref  # noqa: E402
from helpers import golden_graphs, random_family_graphs  # noqa: E402

from desco_amd import _lib, sampling  # noqa: E402
from desco_amd import groundtruth as gt  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 32


def _classes(kmax):
    return [(n, list(e)) for k in range(2, kmax + 1) for n, e in gt.census_classes(k)]


def _small_graphs():
    graphs = golden_graphs(30)
    graphs.append((8, [(a, b) for b in range(8) for a in range(b)]))                         # K8
    graphs.append((13, [(5, i) for i in range(13) if i != 5]))                               # a 12-leaf star
    graphs.append((9, [(i, (i + 1) % 9) for i in range(9)] + [(0, 4), (2, 7), (3, 8)]))      # a 9-cycle with chords
    graphs += [(1, []), (4, [])]                                                             # a single node, no edges
    return graphs


def _host(graphs, queries, level="node", **kw):
    gs = graphs if isinstance(graphs, GraphSet) else GraphSet.from_edge_lists(graphs)
    return sampling.sampled_tallies(gs, queries, backend="host", level=level, **kw).numpy()


SCHEDULES = {"uniform 0.3": lambda kmax: dict(fraction=0.3),
             "(1, 0.5, 1, 0.25, ..)": lambda kmax: dict(probs=(1.0, 0.5, 1.0, 0.25, 0.5)[:kmax - 1]),
             "with a zero": lambda kmax: dict(probs=(0.6, 0.5, 0.0, 1.0, 1.0)[:kmax - 1] if kmax > 3 else (0.6, 0.0))}


@pytest.mark.parametrize("kmax", [3, 4, 5, 6])
@pytest.mark.parametrize("name", list(SCHEDULES))
def test_twin_equals_the_python_reference(kmax, name):
    kw = SCHEDULES[name](kmax)
    graphs, classes = _small_graphs(), _classes(kmax)
    thr = [int(x) for x in sampling.schedule(kmax, **kw)[0]]
    got = _host(graphs, classes, replicas=2, seed=5, graph_base=3, replica_base=7, **kw)
    want = ref.tallies(graphs, classes, thr, 2, seed=5, graph_base=3, replica_base=7)
    assert got.shape == want.shape and got.sum() > 0
    assert np.array_equal(got, want)
    assert sampling.last_backend == "host"


def test_empty_set_and_no_replicas():
    empty = GraphSet.from_edge_lists([])
    assert _host(empty, None, fraction=0.5, replicas=3).shape == (3, 0, 30)
    assert _host(empty, None, fraction=0.5, replicas=3, level="graph").shape == (3, 0, 30)
    assert _host(_small_graphs(), None, fraction=0.5, replicas=0, level="graph").shape == (0, len(_small_graphs()), 30)


@pytest.mark.parametrize("kmax", [5, 6])
def test_all_ones_is_the_exact_count(kmax):
    gs = GraphSet.from_edge_lists(_small_graphs() + random_family_graphs(3, 6))
    exact = gt._induced_host_int64(gs, _classes(kmax), 0)
    got = _host(gs, _classes(kmax), probs=[1.0] * (kmax - 1), replicas=3, seed=9)
    for r in range(3):
        assert np.array_equal(got[r], exact)
    per_graph = _host(gs, _classes(kmax), probs=[1.0] * (kmax - 1), replicas=1, level="graph")[0]
    assert np.array_equal(per_graph, np.add.reduceat(exact, gs.graph_ptr[:-1], axis=0))


def test_prefix():
    gs = GraphSet.from_edge_lists(_small_graphs())
    probs = (0.8, 0.6, 0.7, 0.5)
    sizes = np.array([n for n, _ in _classes(5)])
    whole = _host(gs, _classes(5), probs=probs, replicas=3, seed=2)
    for j in (2, 3, 4):
        part = _host(gs, _classes(j), probs=probs[:j - 1], replicas=3, seed=2)
        assert np.array_equal(part, whole[:, :, sizes <= j]), j
    # a zero at level d zeroes exactly the sizes >= d
    for d in (2, 3, 4, 5):
        p = [0.8, 0.6, 0.7, 0.5]
        p[d - 2] = 0.0
        t = _host(gs, _classes(5), probs=p, replicas=3, seed=2)
        assert np.array_equal(t[:, :, sizes < d], whole[:, :, sizes < d]), d
        assert t[:, :, sizes >= d].sum() == 0 and (d == 2 or t[:, :, sizes < d].sum() > 0), d


def test_monotone_coupling():
    gs = GraphSet.from_edge_lists(_small_graphs())
    rng = np.random.default_rng(4)
    for _ in range(20):
        hi = rng.random(4)
        lo = hi * np.where(rng.random(4) < 0.5, 1.0, rng.random(4))          # some levels lowered, some kept
        assert (sampling.schedule(5, probs=lo)[0] <= sampling.schedule(5, probs=hi)[0]).all()
        a = _host(gs, None, probs=lo, replicas=2, seed=6)
        b = _host(gs, None, probs=hi, replicas=2, seed=6)
        assert (a <= b).all()


def test_slices_and_threads():
    graphs = _small_graphs()
    gs = GraphSet.from_edge_lists(graphs)
    kw = dict(fraction=0.3, seed=8)
    whole = _host(gs, None, replicas=6, num_threads=1, **kw)
    for nt in (3, 16):
        assert np.array_equal(_host(gs, None, replicas=6, num_threads=nt, **kw), whole)
    a, b = 3, 9
    n0, n1 = int(gs.graph_ptr[a]), int(gs.graph_ptr[b])
    assert np.array_equal(_host(gs.subset(a, b), None, replicas=6, graph_base=a, **kw), whole[:, n0:n1])
    assert np.array_equal(_host(gs, None, replicas=3, replica_base=2, **kw), whole[2:5])
    per_graph = _host(gs, None, replicas=6, level="graph", **kw)
    assert np.array_equal(per_graph, np.add.reduceat(whole, gs.graph_ptr[:-1], axis=1))
    # duplicates and isomorphic queries get equal columns
    q = [(3, [(0, 1), (1, 2)]), (3, [(0, 2), (2, 1)]), (3, [(0, 1), (1, 2)]), (2, [(0, 1)])]
    t = _host(gs, q, probs=(0.3 ** 0.25, 0.3 ** 0.25), replicas=6, seed=8)
    assert np.array_equal(t[:, :, 0], t[:, :, 1]) and np.array_equal(t[:, :, 0], t[:, :, 2])
    assert np.array_equal(t[:, :, 0], whole[:, :, 1]) and np.array_equal(t[:, :, 3], whole[:, :, 0])


# ---- unbiasedness: |mean - exact * P| <= 5.5 s / sqrt(R) for every class with an expected tally of at least 20 --------
R_STAT = 1024


@pytest.fixture(scope="module")
def unbiased_data():
    gs = GraphSet.from_edge_lists(random_family_graphs(11, 44))
    assert 36 <= gs.num_graphs <= 44
    thr, probs, _ = sampling.schedule(5, fraction=0.2)
    sizes = np.array([n for n, _ in _classes(5)])
    exact = gt._induced_host_int64(gs, _classes(5), 0).sum(axis=0).astype(np.float64)
    totals = _host(gs, None, fraction=0.2, replicas=R_STAT, seed=2024, level="graph").sum(axis=1).astype(np.float64)
    return sizes, probs, exact, totals


def _gate(sizes, probs, exact, totals, shift=0):
    """(classes that qualify, classes that miss the gate); ``shift``: the survival probability of size k is taken as
    that of size k + shift (the wrong weights)"""
    P = np.array([np.prod(probs[:max(k + shift, 1) - 1]) for k in sizes])
    qualify = exact * P >= 20
    mean, s = totals.mean(axis=0), totals.std(axis=0, ddof=1)
    miss = qualify & ~(np.abs(mean - exact * P) <= 5.5 * s / np.sqrt(totals.shape[0]))
    return qualify, miss


def test_unbiased(unbiased_data):
    sizes, probs, exact, totals = unbiased_data
    qualify, miss = _gate(sizes, probs, exact, totals)
    z = (totals.mean(axis=0) - exact * np.array([np.prod(probs[:k - 1]) for k in sizes])) / \
        np.maximum(totals.std(axis=0, ddof=1) / np.sqrt(R_STAT), 1e-300)
    print(f"[sampled] {int(qualify.sum())} classes qualify; largest |z| = {np.abs(z[qualify]).max():.2f}")
    assert qualify.sum() >= 20 and set(sizes[qualify]) == {2, 3, 4, 5}
    assert not miss.any(), (np.flatnonzero(miss), z[miss])


def test_the_gate_catches_weights_shifted_by_one_level(unbiased_data):
    sizes = unbiased_data[0]
    qualify, miss = _gate(*unbiased_data, shift=-1)              # every size weighted as the size below it
    assert qualify.sum() >= 20 and miss[qualify].all()
    qualify, miss = _gate(*unbiased_data, shift=1)               # .. as the size above it (5 has none above: unchanged)
    assert (qualify & (sizes < 5)).sum() >= 5 and miss[qualify & (sizes < 5)].all()


def test_leaf_decisions_have_binomial_variance():
    f = 0.25
    graphs = [(14, [(a, b) for b in range(14) for a in range(b)]),                           # K14: C(14, 5) = 2002
              (21, [(20, i) for i in range(20)]),                                            # a 20-leaf star: 4845
              random_family_graphs(5, 11)[9]]                                                # G(n, 0.2)
    gs = GraphSet.from_edge_lists(graphs)
    sizes = np.array([n for n, _ in _classes(5)])
    n5 = np.add.reduceat(gt._induced_host_int64(gs, _classes(5), 0), gs.graph_ptr[:-1], axis=0)[:, sizes == 5].sum(axis=1)
    assert (n5 >= 1000).all(), n5
    t = _host(gs, None, probs=(1, 1, 1, f), replicas=R_STAT, seed=77, level="graph")[:, :, sizes == 5].sum(axis=2)
    ratio = t.var(axis=0, ddof=1) / (n5 * f * (1 - f))
    print(f"[sampled] n5 = {n5.tolist()}, variance / binomial variance = {np.round(ratio, 3).tolist()}")
    assert ((ratio >= 0.75) & (ratio <= 1.33)).all()
    assert (np.abs(t.mean(axis=0) - n5 * f) <= 5.5 * np.sqrt(n5 * f * (1 - f) / R_STAT)).all()


# ---- the estimator ----------------------------------------------------------------------------------------------------------
def test_schedule():
    thr, probs, w = sampling.schedule(5, probs=(1.0, 0.5, 0.0, 0.25))
    assert thr.dtype == np.int64 and thr.tolist() == [0, 0, ONE, ONE // 2, 0, ONE // 4]
    assert probs.tolist() == [1.0, 0.5, 0.0, 0.25] and w[:4].tolist() == [1.0, 1.0, 1.0, 2.0] and np.isinf(w[4:]).all()
    thr, probs, w = sampling.schedule(4, fraction=0.001)
    assert thr[2] == thr[3] == int(0.001 ** (1 / 3) * ONE) and w[4] == pytest.approx(1000.0, rel=1e-8)
    assert sampling.schedule(3, fraction=1.0)[0].tolist() == [0, 0, ONE, ONE]
    for bad in (dict(), dict(fraction=0.5, probs=(0.5, 0.5)), dict(fraction=1.5), dict(fraction=-0.1),
                dict(probs=(0.5, 1.5)), dict(probs=(-0.5, 0.5)), dict(probs=(0.5,))):
        with pytest.raises(ValueError):
            sampling.schedule(3, **bad)
    with pytest.raises(ValueError):
        sampling.schedule(7, fraction=0.5)


def test_estimate_counts():
    gs = GraphSet.from_edge_lists(_small_graphs())
    kw = dict(fraction=0.4, replicas=8, seed=1, backend="host")
    est = sampling.estimate_counts(gs, None, **kw)
    sizes = np.array([n for n, _ in est.columns])
    assert est.estimate.shape == est.stderr.shape == (gs.num_graphs, 30) and est.tallies.shape == (8, gs.num_graphs, 30)
    x = est.tallies * est.weights[sizes]
    assert np.allclose(est.estimate, x.mean(axis=0), rtol=1e-13)
    assert np.allclose(est.stderr, x.std(axis=0, ddof=1) / np.sqrt(8), rtol=1e-13)
    assert est.last_backend == "host" and len(est.probs) == 4
    t = est.table()
    assert list(t) == ["graph", "query", "estimate", "stderr"] and len(t["graph"]) == gs.num_graphs * 30
    assert t["estimate"][31] == est.estimate[1, 1]
    # non-induced = noninduced_matrix applied to the induced estimates of the whole census of the size
    for k in (3, 4, 5):
        cols = np.flatnonzero(sizes == k)
        queries = [est.columns[i] for i in cols]
        non = sampling.estimate_counts(gs, queries, induced=False, probs=est.probs[:k - 1], replicas=8, seed=1,
                                       backend="host")
        want = est.estimate[:, cols] @ gt.noninduced_matrix(k).T.astype(np.float64)
        assert np.allclose(non.estimate, want, rtol=1e-12, atol=1e-9)
        assert (non.stderr >= 0).all()
    one = sampling.estimate_counts(gs, None, fraction=0.4, replicas=1, backend="host")
    assert np.isnan(one.stderr).all() and np.isfinite(one.estimate).all()
    node = sampling.estimate_counts(gs, [(3, [(0, 1), (1, 2), (0, 2)])], fraction=1.0, replicas=2, backend="host",
                                    level="node")
    assert np.array_equal(node.estimate[:, 0], gt._induced_host_int64(gs, [(3, [(0, 1), (1, 2), (0, 2)])], 0)[:, 0])
    assert (node.stderr == 0).all()
    with pytest.raises(RuntimeError, match="2..6 nodes"):
        sampling.sampled_tallies(gs, [(7, [(i, i + 1) for i in range(6)])], fraction=0.5, backend="host")
    with pytest.raises(ValueError):
        sampling.sampled_tallies(gs, None, probs=(0.5, 0.5), backend="host")      # 30 classes need 4 levels


# ---- the entry points ---------------------------------------------------------------------------------------------------------
HOST, DEV = "desco_sampled_counts", "desco_sampled_counts_dev"


def test_entry_points_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "desco_hip.h")).read()
    assert "SAMPLED COUNTS" in src
    for name in (HOST, DEV):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m and hasattr(_lib.lib(), name) and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(","))
    assert _lib.lib().desco_abi_version() == 6


BUF = np.zeros(4096, np.int64)          # host memory: every device call below must fail its argument check (no launch)
P = BUF.ctypes.data
THR = np.array([0, 0, ONE, ONE, ONE, ONE, ONE], dtype=np.int64)


def _host_call(**over):
    gs = GraphSet.from_edge_lists([(3, [(0, 1), (1, 2)])])
    _, q_nodes, q_edge_ptr, q_edges = gt._flatten_queries([(2, [(0, 1)]), (3, [(0, 1), (1, 2)])])
    thr = over.pop("thr_values", THR)
    args = dict(graph_ptr=gs.graph_ptr.ctypes.data, num_graphs=1, rowptr=gs.rowptr.ctypes.data, col=gs.col.ctypes.data,
                q_nodes=q_nodes.ctypes.data, q_edge_ptr=q_edge_ptr.ctypes.data, q_edges=q_edges.ctypes.data,
                num_queries=2, kmax=3, thr=thr.ctypes.data, seed=0, graph_base=0, replica_base=0, num_replicas=1,
                per_graph=0, num_threads=1, out=P)
    args.update(over)
    return _lib.lib().desco_sampled_counts(*args.values())


def _dev_call(**over):
    thr = over.pop("thr_values", THR)
    args = dict(graph_ptr=P, num_graphs=1, num_nodes=3, rowptr=P, num_entries=4, col=P, node_graph=P, bit_off=P, bits=P,
                num_words=3, cls=P, kmax=3, num_queries=2, thr=thr.ctypes.data, seed=0, graph_base=0, replica_base=0,
                num_replicas=1, per_graph=0, out=P, stream=None)
    args.update(over)
    return _lib.lib().desco_sampled_counts_dev(*args.values())


def test_entry_points_reject_bad_arguments():
    L = _lib.lib()
    bad_thr = [np.array([0, 0, ONE, ONE + 1], dtype=np.int64), np.array([0, 0, -1, ONE], dtype=np.int64)]
    assert _host_call() == 0 and BUF[:6].tolist() == [0, 0, 1, 0, 1, 1]           # (the valid call: P3 0 - 1 - 2)
    for over in [dict(graph_ptr=None), dict(rowptr=None), dict(col=None), dict(q_nodes=None), dict(q_edge_ptr=None),
                 dict(thr=None), dict(out=None), dict(kmax=1), dict(kmax=7), dict(kmax=2), dict(num_queries=-1),
                 dict(num_replicas=-1), dict(graph_base=-1), dict(replica_base=-1), dict(num_graphs=-1),
                 dict(per_graph=2)] + [dict(thr_values=t) for t in bad_thr]:
        assert _host_call(**over) == -1, over
        assert HOST.encode() + b":" in L.desco_last_error(), over
    for over in [dict(graph_ptr=None), dict(rowptr=None), dict(col=None), dict(node_graph=None), dict(bit_off=None),
                 dict(bits=None), dict(cls=None), dict(thr=None), dict(out=None), dict(kmax=1), dict(kmax=6),
                 dict(num_queries=33), dict(num_queries=-1), dict(num_replicas=-1), dict(num_nodes=-1),
                 dict(num_entries=-1), dict(graph_base=-1), dict(replica_base=-1), dict(per_graph=2),
                 dict(per_graph=1, num_graphs=0), dict(num_entries=1 << 40, num_replicas=1 << 20)] + [dict(thr_values=t) for t in bad_thr]:
        assert _dev_call(**over) == -1, over
        assert DEV.encode() + b":" in L.desco_last_error(), over
    assert _dev_call(num_entries=1 << 40, num_replicas=1 << 20) == -1 and b"work items" in L.desco_last_error()
    assert _dev_call(thr_values=bad_thr[0]) == -1 and b"threshold" in L.desco_last_error()
    # nothing to do: 0 before any pointer is looked at
    assert _dev_call(num_replicas=0, graph_ptr=None) == 0 and _dev_call(num_nodes=0, out=None) == 0
    assert _dev_call(num_queries=0, cls=None) == 0
    assert _host_call(num_replicas=0, out=None) == 0 and _host_call(num_graphs=0, graph_ptr=None) == 0


# ---- the driver ---------------------------------------------------------------------------------------------------------------
def test_driver_end_to_end(tmp_path):
    import sampled_counts as D
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = D.main(["--datasets", "MUTAG", "--fraction", "0.2", "--replicas", "4", "--query_size", "3", "4",
                      "--backend", "host", "--compare_exact", "--output_dir", str(tmp_path),
                      "--data_root", str(tmp_path / "none")])
        again = D.main(["--datasets", "MUTAG", "--probs", "1", "1", "1", "--replicas", "2", "--query_size", "3", "4",
                        "--noninduced", "--backend", "host", "--compare_exact", "--output_dir", str(tmp_path),
                        "--data_root", str(tmp_path / "none")])
    assert os.path.basename(out["csv"]) == "sampled-counts_0.csv"
    assert os.path.basename(again["csv"]) == "sampled-counts_1.csv"
    info = out["datasets"]["MUTAG"]
    assert info["backend"] == "host" and len(info["norm_mse"]) == len(info["mae"]) == 2
    assert all(np.isfinite(info["norm_mse"])) and info["sampled_seconds"] > 0 and info["exact_seconds"] > 0
    with open(out["csv"], newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["dataset", "graph", "query", "estimate", "stderr", "exact"]
    assert len(rows) == 1 + 188 * 8 and rows[1][:3] == ["MUTAG", "0", "0"]
    # probability 1 everywhere: the estimate is the exact (non-induced) count and the error bar is 0
    assert again["datasets"]["MUTAG"]["mae"] == [0.0, 0.0]
    with open(again["csv"], newline="") as f:
        rows = list(csv.reader(f))[1:]
    assert all(float(r[3]) == float(r[5]) and float(r[4]) == 0.0 for r in rows)
