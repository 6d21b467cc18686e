"""The host twin of the graph generators (csrc/graph_gen.cpp) against the plain Python evaluation of the definition
(tests/graph_gen_reference.py), its invariants, its fidelity to networkx's generators, the schedules and the driver."""
import math
import os
import random
import subprocess
import sys

import networkx as nx
import numpy as np
import pytest
from scipy import stats

import graph_gen_reference as R
from desco_amd import generators as G
from test_oracle_dropout import KAT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T32 = 1 << 32
SIZES = (1, 2, 3, 10, 32, 33, 64, 65, 130)
ALPHA = 1e-6                    # a statistic has to lie below the 1 - ALPHA quantile of its null distribution


def targets(n):
    top = n * (n - 1) // 2
    return [max(min(e, top), n - 1) for e in (n - 1, 2 * n, n * n // 4, top)]


def assert_same(a, b):
    for name in ("graph_ptr", "rowptr", "col", "deg", "status"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def reference(spec):
    return G.Generated(*R.generate(spec.family, spec.n, spec.param, spec.threshold, spec.seed, spec.graph_base), "ref")


def spec_of(rows, seed=3, graph_base=0, flags=0):
    f, n, p0, p1, t0, t1 = zip(*rows)
    return G._Spec(f, n, np.array([p0, p1], dtype=np.int64).T, np.array([t0, t1], dtype=np.uint64).T, seed,
                   graph_base, flags)


def all_families_spec(seed=5, graph_base=0):
    cases = [(f, n, e) for f in range(6) for n in (1, 2, 7, 33, 70) for e in targets(n)[:3]]
    f, n, e = zip(*cases)
    return G._spec(f, n, e, seed, graph_base)


# ---- the draws --------------------------------------------------------------------------------------------------------

def test_philox_known_answers_and_the_exposed_draw():
    for ctr, key, want in KAT:
        assert R.philox4x32_10(ctr, key) == want
    for seed, graph, stream, i, bound in ((0, 0, 0, 0, 1), (12345678901234567, 4000000000, 3, 9, 977),
                                          ((1 << 64) - 1, 17, 115, (1 << 40) + 6, (1 << 32) - 1)):
        w = R.word(seed, graph, stream, i)
        assert G.draw(seed, graph, stream, i, bound) == (w, (w * bound) >> 32)


# ---- twin == reference ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", range(6), ids=G.FAMILIES)
def test_twin_equals_the_reference(family):
    cases = [(family, n, e) for n in SIZES for e in targets(n)]
    f, n, e = zip(*cases)
    for seed, base in ((0, 0), (977, 41), ((1 << 63) + 12345, (1 << 32) - len(cases))):
        keep = slice(None) if seed == 0 else slice(0, 24)          # (the largest shapes once)
        spec = G._spec(f[keep], n[keep], e[keep], seed, base)
        assert_same(G._host(spec, 2), reference(spec))


def test_twin_equals_the_reference_on_the_hard_parameter_corners():
    rows = [(G.ER, 200, 0, 0, G.threshold(100 / 19900), 0)]                                  # hundreds of components
    rows += [(G.WS, n, 2, n, T32, 0) for n in (12, 20, 30) for _ in range(4)]                # retries
    rows += [(G.WS, n, k, n + 3, T32, 0) for n in (2, 12) for k in (0, 1)]                   # the fallback
    rows += [(G.RANDOM, 20, 171, 0, 0, 0)]
    for n, m in ((12, 2), (20, 5), (33, 1)):
        rows += [(G.EBA, n, m, 0, int(0.5 * T32), int(0.95 * T32)), (G.EBA, n, m, 0, int(0.05 * T32), int(0.9 * T32))]
    rows += [(G.POWER, 10, 1, 0, T32 // 2, 0), (G.POWER, 40, 5, 0, T32, 0), (G.POWER, 12, 12, 0, T32, 0)]
    spec = spec_of(rows, seed=7)
    h = G._host(spec, 3)
    assert_same(h, reference(spec))
    tries = h.status & 0xff
    assert ((tries > 1) & (tries <= 100)).any() and (tries == G.WS_FELL_BACK).any()
    assert (h.status[0] >> 8) >= 50
    for flags in (G.NO_CONNECT, G.NO_RELABEL, G.NO_CONNECT | G.NO_RELABEL):
        assert G._host(spec_of(rows, 7, 0, flags), 1).status.tolist() == [
            s & 0xff if flags & G.NO_CONNECT else s for s in h.status]


# ---- independence -----------------------------------------------------------------------------------------------------

def test_threads_and_slices_do_not_change_a_bit():
    spec = all_families_spec()
    one, four = G._host(spec, 1), G._host(spec, 4)
    assert_same(one, four)
    ids = np.arange(spec.G, dtype=np.int64)
    cut = 37
    a, b = G._host(spec.subset(ids[:cut]), 2), G._host(spec.subset(ids[cut:]), 2)
    assert np.array_equal(np.concatenate([a.deg, b.deg]), one.deg)
    assert np.array_equal(np.concatenate([a.status, b.status]), one.status)
    assert np.array_equal(np.concatenate([a.col, b.col + one.graph_ptr[cut]]), one.col)
    other = G._host(all_families_spec(seed=6), 4)
    assert not np.array_equal(other.col, one.col)


# ---- invariants -------------------------------------------------------------------------------------------------------

def check_invariants(r):
    gs = r.to_graphset()
    N = gs.num_nodes
    rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(gs.rowptr))
    col = gs.col.astype(np.int64)
    graph_of = gs.node_graph_ids()
    assert (col != rows).all() and (graph_of[col] == graph_of[rows]).all()                  # loop free, inside the graph
    inner = np.ones(len(col), dtype=bool)
    inner[gs.rowptr[:-1][np.diff(gs.rowptr) > 0]] = False
    assert (np.diff(col)[inner[1:]] > 0).all()                                             # rows strictly ascending
    key = rows * N + col
    assert np.array_equal(np.sort(key), np.sort(col * N + rows))                           # symmetric
    assert np.array_equal(np.diff(gs.rowptr), r.deg)
    for n, edges in gs.edge_lists():                                                       # connected
        g = nx.empty_graph(n)
        g.add_edges_from(edges)
        assert n == 1 or nx.is_connected(g)


def test_every_generated_graph_is_simple_symmetric_sorted_and_connected():
    check_invariants(G._host(all_families_spec(), 0))
    fam, n, e = G.schedule(150, 10, 90, seed=3)
    r = G._run(G._spec(fam, n, e, 3, 0), "host", 0)
    assert np.array_equal(np.diff(r.graph_ptr), n)
    check_invariants(r)


def test_edge_counts():
    def edges_of(r):
        return np.diff(r.rowptr[r.graph_ptr]) // 2

    n = np.array([2, 5, 16, 33, 64, 100])
    m = np.array([1, 4, 3, 32, 7, 99])
    r = G.generate_params([G.BA] * 6, n, np.stack([m, 0 * m], 1), np.zeros((6, 2)), seed=1, backend="host")
    assert np.array_equal(edges_of(r), m * (n - m)) and (r.added == 0).all()
    k = np.array([1, 4, 6, 2, 10, 20])
    r = G.generate_params([G.WS] * 6, n, np.stack([np.minimum(k, n - 1), n], 1), [[G.threshold(0.1), 0]] * 6, seed=2,
                          backend="host")
    first = (r.tries >= 1) & (r.tries <= 100)
    assert first.sum() >= 4
    assert np.array_equal(edges_of(r)[first], (n * (np.minimum(k, n - 1) // 2))[first]) and (r.added[first] == 0).all()
    m = np.array([1, 3, 20, 40, 500, 120])
    r = G.generate_params([G.RANDOM] * 6, n, np.stack([m, 0 * m], 1), np.zeros((6, 2)), seed=3, backend="host")
    assert np.array_equal(edges_of(r), m + r.added) and (r.added > 0).any()
    body = G.generate_params([G.RANDOM] * 6, n, np.stack([m, 0 * m], 1), np.zeros((6, 2)), seed=3, backend="host",
                             flags=G.NO_CONNECT).to_graphset()
    comps = []
    for k, e in body.edge_lists():
        g = nx.empty_graph(k)
        g.add_edges_from(e)
        comps.append(nx.number_connected_components(g))
    assert np.array_equal(r.added, np.array(comps) - 1)


def test_the_complete_graph_cases_come_out_complete():
    rows = []
    for n in (2, 5, 8, 9, 33):
        top = n * (n - 1) // 2
        rows += [(G.ER, n, 0, 0, T32, 0), (G.RANDOM, n, top, 0, 0, 0), (G.RANDOM, n, top + 5, 0, 0, 0)]
        if n > 2:
            rows += [(G.WS, n, n - 1, top, T32, 0)] if n % 2 else []          # k = n - 1 even: the lattice is complete
    r = G._host(spec_of(rows), 0)
    n = np.diff(r.graph_ptr)
    assert np.array_equal(np.diff(r.rowptr[r.graph_ptr]), n * (n - 1))
    # k = n - 1 on even n: every node lacks its antipode alone; n (n - 2) / 2 edges stand whatever is rewired
    even = G._host(spec_of([(G.WS, n, n - 1, 0, T32, 0) for n in (4, 8, 34)]), 0)
    n = np.diff(even.graph_ptr)
    assert np.array_equal(np.diff(even.rowptr[even.graph_ptr]) // 2, n * ((n - 1) // 2))
    # EBA with no room to add (two existing nodes, m = 2): the add is skipped, the growth step alone gives the path
    eba = G._host(spec_of([(G.EBA, 3, 2, 0, T32, T32)] * 5), 0)
    assert (eba.deg.reshape(5, 3).sum(1) == 4).all()


# ---- fidelity to networkx ---------------------------------------------------------------------------------------------

def eba_restated(n, m, p, q, rng):
    """The extended Barabasi-Albert model with its attachment list, on random.Random; an empty choice ends the step."""
    adj = {v: set() for v in range(m)}
    pref = list(range(m))
    for new in range(m, n):
        a = rng.random()
        full = len(adj) - 1
        room = len(adj) * full / 2
        size = sum(len(x) for x in adj.values()) // 2
        try:
            if a < p and size <= room - m:
                eligible = [v for v in adj if len(adj[v]) < full]
                for _ in range(m):
                    src = rng.choice(eligible)
                    dst = rng.choice([v for v in pref if v != src and v not in adj[src]])
                    adj[src].add(dst), adj[dst].add(src)
                    pref += [src, dst]
                    if len(adj[src]) == full:
                        eligible.remove(src)
                    if len(adj[dst]) == full and dst in eligible:
                        eligible.remove(dst)
            elif p <= a < p + q and m <= size < room:
                eligible = [v for v in adj if 0 < len(adj[v]) < full]
                for _ in range(m):
                    node = rng.choice(eligible)
                    old = rng.choice(sorted(adj[node]))
                    dst = rng.choice([v for v in pref if v != node and v not in adj[node]])
                    adj[node].remove(old), adj[old].remove(node)
                    adj[node].add(dst), adj[dst].add(node)
                    pref.remove(old)
                    pref.append(dst)
                    if len(adj[old]) == 0 and old in eligible:
                        eligible.remove(old)
                    if dst in eligible:
                        if len(adj[dst]) == full:
                            eligible.remove(dst)
                    elif len(adj[dst]) == 1:
                        eligible.append(dst)
        except IndexError:
            pass
        chosen = set()
        while len(chosen) < m:
            chosen.add(rng.choice(pref))
        adj[new] = set(chosen)
        for v in chosen:
            adj[v].add(new)
        pref += list(chosen) + [new] * (m + 1)
    return [(u, v) for u in adj for v in adj[u] if u < v]


def power_restated(n, m, p, rng):
    """Holme-Kim growth in which a triangle edge does not count towards m, on random.Random; the m targets of a node are
    used in the order in which they were drawn."""
    adj = {v: set() for v in range(m)}
    repeated = list(range(m))
    for source in range(m, n):
        targets_ = []
        while len(targets_) < m:
            x = rng.choice(repeated)
            if x not in targets_:
                targets_.append(x)
        adj[source] = set()

        def link(x):
            adj[source].add(x), adj[x].add(source)
            repeated.append(x)

        target = targets_.pop(0)
        link(target)
        count = 1
        while count < m:
            if rng.random() < p:
                near = [x for x in sorted(adj[target]) if x != source and x not in adj[source]]
                if near:
                    link(rng.choice(near))
                    continue
            target = targets_.pop(0)
            link(target)
            count += 1
        repeated += [source] * m
    return [(u, v) for u in adj for v in adj[u] if u < v]


def other_sample(family, n, a, p, q, count, seed):
    """`count` edge lists of the family from networkx (restated for EBA and Power), one seeded stream"""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        if family == G.ER:
            out.append(list(nx.gnp_random_graph(n, p, seed=rng).edges()))
        elif family == G.WS:
            out.append(list(nx.connected_watts_strogatz_graph(n, a, p, tries=100, seed=rng).edges()))
        elif family == G.RANDOM:
            out.append(list(nx.gnm_random_graph(n, a, seed=rng).edges()))
        elif family == G.BA:
            out.append(list(nx.barabasi_albert_graph(n, a, seed=rng).edges()))
        elif family == G.EBA:
            out.append(eba_restated(n, a, p, q, rng))
        else:
            out.append(power_restated(n, a, p, rng))
    return out


def twin_sample(family, n, a, p, q, count, seed):
    rows = [(family, n, a, 0, G.threshold(p), G.threshold(p + q) if family == G.EBA else 0)] * count
    gs = G._host(spec_of(rows, seed, 0, G.NO_CONNECT | G.NO_RELABEL), 0).to_graphset()
    return [e for _, e in gs.edge_lists()]


def masks(sample):
    return np.array([sum(1 << (max(u, v) * (max(u, v) - 1) // 2 + min(u, v)) for u, v in edges) for edges in sample])


def chi_square(a, b):
    """two-sample chi-square statistic of two equally large samples of labels and the 1 - ALPHA quantile of its null
    distribution; cells in which the two samples together hold fewer than 10 are pooled (expected count >= 5 each)"""
    assert len(a) == len(b)
    keys, inv = np.unique(np.concatenate([a, b]), return_inverse=True)
    ca = np.bincount(inv[:len(a)], minlength=len(keys)).astype(float)
    cb = np.bincount(inv[len(a):], minlength=len(keys)).astype(float)
    small = ca + cb < 10
    if small.any():
        ca, cb = np.append(ca[~small], ca[small].sum()), np.append(cb[~small], cb[small].sum())
        if ca[-1] + cb[-1] < 10 and len(ca) > 1:          # the pooled cell joins its neighbour
            ca[-2] += ca[-1]
            cb[-2] += cb[-1]
            ca, cb = ca[:-1], cb[:-1]
    cells = len(ca)
    if cells < 2:
        return 0.0, 1.0, cells
    stat = float(((ca - cb) ** 2 / (ca + cb)).sum())
    return stat, float(stats.chi2.ppf(1 - ALPHA, cells - 1)), cells


SMALL = {G.ER: ((0, 0.3, 0), (0, 0.6, 0)), G.WS: ((2, 0.5, 0), (4, 0.3, 0)), G.RANDOM: ((3, 0, 0), (7, 0, 0)),
         G.BA: ((1, 0, 0), (2, 0, 0)), G.EBA: ((1, 0.3, 0.3), (2, 0.5, 0.2)), G.POWER: ((2, 0.5, 0), (3, 1.0, 0))}


@pytest.mark.parametrize("family", range(6), ids=G.FAMILIES)
def test_labelled_edge_sets_are_distributed_as_networkx_draws_them(family):
    count = 4000
    for n in (5, 6):
        for a, p, q in SMALL[family]:
            if family == G.WS and a >= n - 1:
                a = 2 if p > 0.4 else 3                   # (n = 5: k = 4 would be the complete lattice)
                p = 0.1 if a == 3 else p
            if n == 6 and family == G.ER and p > 0.5:
                p = 0.12                                  # (2^15 edge sets: a sparse setting keeps cells above the pool)
            if n == 6 and family == G.RANDOM and a == 7:
                a = 2
            ours = masks(twin_sample(family, n, a, p, q, count, seed=100 + n))
            theirs = masks(other_sample(family, n, a, p, q, count, seed=200 + n))
            again = masks(other_sample(family, n, a, p, q, count, seed=300 + n))
            stat, bound, cells = chi_square(ours, theirs)
            stat0, bound0, _ = chi_square(theirs, again)
            print(f"{G.FAMILIES[family]} n={n} a={a} p={p} q={q}: chi2 {stat:.1f} < {bound:.1f} over {cells} cells; "
                  f"networkx against itself {stat0:.1f} < {bound0:.1f}")
            assert cells >= 4
            assert stat0 < bound0                          # the yardstick holds the other generator against itself
            assert stat < bound


def ks_bound(count):
    """Smirnov's asymptotic 1 - ALPHA quantile of the two-sample statistic for two samples of `count`"""
    return math.sqrt(-math.log(ALPHA / 2) / 2) * math.sqrt(2.0 / count)


def figures(sample, n):
    out = np.zeros((len(sample), 3))
    for i, edges in enumerate(sample):
        m = np.zeros((n, n))
        if edges:
            e = np.array(edges)
            m[e[:, 0], e[:, 1]] = m[e[:, 1], e[:, 0]] = 1
        out[i] = len(edges), np.trace(m @ m @ m) / 6, m.sum(0).max()
    return out


LARGE = {G.ER: (0, 0.08, 0), G.WS: (6, 0.1, 0), G.RANDOM: (150, 0, 0), G.BA: (3, 0, 0), G.EBA: (2, 0.3, 0.1),
         G.POWER: (4, 0.4, 0)}


@pytest.mark.parametrize("family", range(6), ids=G.FAMILIES)
def test_edge_triangle_and_degree_figures_at_60_nodes_follow_networkx(family):
    count, n = 600, 60
    a, p, q = LARGE[family]
    ours = figures(twin_sample(family, n, a, p, q, count, seed=400), n)
    theirs = figures(other_sample(family, n, a, p, q, count, seed=500), n)
    again = figures(other_sample(family, n, a, p, q, count, seed=600), n)
    bound = ks_bound(count)
    for c, name in enumerate(("edges", "triangles", "largest degree")):
        d = stats.ks_2samp(ours[:, c], theirs[:, c]).statistic
        d0 = stats.ks_2samp(theirs[:, c], again[:, c]).statistic
        print(f"{G.FAMILIES[family]} {name}: KS {d:.4f} < {bound:.4f}; networkx against itself {d0:.4f}")
        assert d0 < bound
        assert d < bound


# ---- uniformity -------------------------------------------------------------------------------------------------------

def test_the_relabelling_is_uniform_over_the_24_permutations_of_4_nodes():
    count = 6000
    perms = np.array([np.argsort([G.draw(9, g, G.STREAM_RELABEL, v)[0] for v in range(4)], kind="stable") @ (4 ** np.arange(4))
                      for g in range(count)])
    assert len(np.unique(perms)) == 24
    stat = float(((np.unique(perms, return_counts=True)[1] - count / 24) ** 2 / (count / 24)).sum())
    assert stat < stats.chi2.ppf(1 - ALPHA, 23), stat
    # and the twin applies that rank: a path 0-1-2-3 (WS k = 2 with no rewiring, one edge short) is too symmetric to
    # show it, so the test above compares whole graphs with the reference instead


def test_the_connecting_tree_is_uniform_over_the_16_labelled_trees_on_4_components():
    count = 6000
    r = G._host(spec_of([(G.ER, 4, 0, 0, 0, 0)] * count, seed=10, flags=G.NO_RELABEL), 0)      # four isolated nodes
    assert (r.added == 3).all()
    trees = masks([e for _, e in r.to_graphset().edge_lists()])
    labels, counts = np.unique(trees, return_counts=True)
    assert len(labels) == 16
    stat = float(((counts - count / 16) ** 2 / (count / 16)).sum())
    assert stat < stats.chi2.ppf(1 - ALPHA, 15), stat


# ---- schedules --------------------------------------------------------------------------------------------------------

def test_schedules():
    fam, n, e = G.schedule(1827)
    sid = np.arange(1380)
    assert np.array_equal(n[:1380], sid // 23 + 10)
    base = 5 * ((np.arange(1380, 1827) - 1380) // 3) + 60
    assert (np.abs(n[1380:] - base) <= 5).all()
    n64 = n.astype(np.int64)
    assert (e >= n64 - 1).all() and (e <= n64 * (n64 - 1) // 2).all()
    assert set(fam) == set(range(6)) and np.bincount(fam).min() > 1827 / 6 * 0.7
    mean_degree = e[:1380] / n64[:1380]
    assert np.corrcoef(mean_degree, 0.5 * (sid % 23) + 1)[0, 1] > 0.9
    again = G.schedule(1827)
    assert all(np.array_equal(x, y) for x, y in zip((fam, n, e), again))
    for count, lo, hi in ((300, 10, 500), (64, 5, 9)):
        fam, n, e = G.schedule(count, lo, hi, seed=1)
        n64 = n.astype(np.int64)
        assert len(n) == count and (n >= lo).all() and (n < hi).all()
        assert (e >= n64 - 1).all() and (e <= n64 * (n64 - 1) // 2).all()
    assert not np.array_equal(G.schedule(300, seed=1)[1], G.schedule(300, seed=2)[1])
    small = G.gen_synthetic(40, 10, 60, seed=2, backend="host")
    assert small.num_graphs == 40 and G.last_backend == "host"
    assert (G.workspace_words(np.array([1, 32, 33, 1056, 1057])) == [9, 164, 235, 39076, 41227]).all()
    for f in range(6):
        for nn in (1, 2, 3, 10, 57, 400):
            for ee in targets(nn):
                p0, p1, t0, t1 = G.family_params(f, nn, ee)
                assert R.ER <= f <= R.POWER and 0 <= t0 <= T32 and 0 <= t1 <= T32 and p0 >= 0 and p1 >= 0


# ---- the driver -------------------------------------------------------------------------------------------------------

def test_gen_dataset_writes_what_load_data_reads(tmp_path):
    from desco_amd.data import load_data, read_syn_edgelist, write_syn_edgelist
    root = str(tmp_path / "data")
    cmd = [sys.executable, os.path.join(ROOT, "gen_dataset.py"), "--dataset", "Syn_12", "--seed", "3", "--depth", "2",
           "--root", root, "--backend", "host"]
    run = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert run.returncode == 0, run.stdout + run.stderr
    raw = os.path.join(root, "Syn_12", "raw")
    stem = os.path.join(raw, "Synthetic_size_min_10_max_500_graph_num_12")
    assert os.path.exists(stem + "_edgelist.txt") and os.path.exists(stem + "_graph_indicator.txt")
    loaded = load_data("Syn_12", root_folder=root)
    made = G.gen_synthetic(12, 10, 500, seed=3, backend="host")
    a, b = str(tmp_path / "e.txt"), str(tmp_path / "i.txt")
    write_syn_edgelist(made, a, b)
    want = read_syn_edgelist(a, b)
    for name in ("graph_ptr", "rowptr", "col"):
        assert np.array_equal(getattr(loaded, name), getattr(want, name)), name
    assert load_data("Syn_12_train", root_folder=root).num_graphs == 3
    truth = os.listdir(os.path.join(root, "Syn_12", "CanonicalCountTruth"))
    assert len(truth) == 1 and truth[0].startswith("query_num_29_query_len_sum_") and truth[0].endswith(".pt")
    before = open(stem + "_edgelist.txt").read()
    run = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert run.returncode == 1 and "not overwritten" in run.stderr
    assert open(stem + "_edgelist.txt").read() == before


# ---- bad arguments ----------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_by_name():
    L = G._lib.lib()

    def refused(what, rows=None, num=None, base=0, null=None, flags=0, t=None, n=None):
        rows = rows or [(G.BA, 5, 2, 0, 0, 0)]
        s = spec_of(rows)
        if n is not None:
            s.n[:] = n
        thr = s.threshold if t is None else np.array(t, dtype=np.uint64)
        bits, deg, st = np.zeros(int(s.bit_ptr[-1]) + 1, np.uint32), np.zeros(64, np.int32), np.zeros(8, np.int32)
        args = [s.family.ctypes.data, s.n.ctypes.data, s.param.ctypes.data, thr.ctypes.data, s.G if num is None else num,
                base, 0, 1, flags, s.graph_ptr.ctypes.data, s.bit_ptr.ctypes.data, bits.ctypes.data, deg.ctypes.data,
                st.ctypes.data]
        if null is not None:
            args[null] = None
        assert L.desco_graph_gen(*args) == -1, what
        msg = L.desco_last_error().decode()
        assert msg.startswith("desco_graph_gen:") and what in msg, msg
        assert not bits.any() and not deg.any() and not st.any()        # refused before anything is written

    refused("negative", num=-1)
    refused("negative", base=-1)
    refused("null pointer", null=0)
    refused("null pointer", null=11)
    refused("unknown family", [(6, 5, 2, 0, 0, 0)])
    refused("unknown family", [(-1, 5, 2, 0, 0, 0)])
    refused("n < 1", [(G.ER, 5, 0, 0, 0, 0)], n=0)
    refused("n < 1", [(G.ER, 5, 0, 0, 0, 0)], n=-3)
    refused("threshold above 2^32", t=[[T32 + 1, 0]])
    refused("threshold above 2^32", t=[[0, 1 << 40]])
    refused("unknown flags", flags=4)
    for family, n, m in ((G.BA, 5, 0), (G.BA, 5, 5), (G.EBA, 5, 0), (G.EBA, 5, 5), (G.POWER, 5, 0), (G.POWER, 5, 6),
                         (G.RANDOM, 5, -1), (G.WS, 5, 5), (G.WS, 5, -2)):
        refused("outside the family's range", [(family, n, m, 0, 0, 0)])
    refused("threshold 0 <= threshold 1", [(G.EBA, 5, 2, 0, 9, 3)])
    assert L.desco_graph_gen(*([None] * 4), 0, 0, 0, 0, 0, None, None, None, None, None) == 0       # nothing to do
    assert L.desco_graph_gen_draw(0, -1, 0, 0, 1, None) == -1 and b"desco_graph_gen_draw" in L.desco_last_error()
    out = np.zeros(2, np.int64)
    assert L.desco_graph_gen_draw(0, 0, 0, 0, T32, out.ctypes.data) == -1 and b"bound" in L.desco_last_error()
    assert L.desco_graph_gen_expand(None, None, None, None, 1, 0, None) == -1
    assert b"desco_graph_gen_expand" in L.desco_last_error()
    assert L.desco_graph_gen_dev(*([None] * 4), 1, None, 0, 0, 0, None, None, 0, 0, 64, 0, 0, None, None, None, None) == -1
    assert b"desco_graph_gen_dev" in L.desco_last_error()
    assert L.desco_graph_gen_dev(*([None] * 4), 1, None, 0, 0, 0, None, None, 0, 0, 40961, 0, 0, None, None, None,
                                 None) == -1
    assert b"DESCO_GRAPH_GEN_DEV_MAX_WORDS" in L.desco_last_error()
    assert L.desco_graph_gen_expand_dev(None, None, None, None, 1, 1, 1, 1, None, None) == -1
    assert b"desco_graph_gen_expand_dev" in L.desco_last_error()
    with pytest.raises(ValueError, match="unknown family"):
        G.generate(["Erdos"], [5], [5])
    with pytest.raises(ValueError, match="unknown backend"):
        G.generate(["ER"], [5], [5], backend="gpu")
    with pytest.raises(ValueError, match="n < 1"):
        G.generate(["ER"], [0], [5], backend="host")
    with pytest.raises(ValueError, match="graph_base"):
        G.generate(["ER"], [5], [5], backend="host", graph_base=1 << 32)


def test_the_ops_wrappers_refuse_cpu_tensors_and_mismatched_arrays():
    import torch
    from desco_amd import ops
    z32, z64 = (lambda k: torch.zeros(k, dtype=torch.int32)), (lambda k: torch.zeros(k, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.graph_gen_dev(z32(1), z32(1), z64(2), z64(2), None, 0, 0, z64(2), z64(2), 64, 0, 0, z32(4), z32(4), z32(1))
    with pytest.raises(ValueError, match="different graph counts"):
        ops.graph_gen_dev(z32(2), z32(1), z64(2), z64(2), None, 0, 0, z64(2), z64(2), 64, 0, 0, z32(4), z32(4), z32(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.graph_gen_expand_dev(z64(2), z64(2), z32(4), z64(5), 0, z32(1))
    with pytest.raises(ValueError, match="shorter"):
        ops.graph_gen_expand_dev(z64(2), z64(2), z32(4), z64(5), 3, z32(1))
