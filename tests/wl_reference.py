"""Yardsticks of the colour-refinement tests, in plain Python.

``exact_refine``: 1-WL refinement with EXACT colours -- a colour is the tuple (own colour, the sorted multiset of the
neighbours' colours per group), interned to an integer per round across the whole input, so two rows get one id iff their
tuples are equal; nothing is hashed.  The same initial colours and the same signature structure as the definition in
include/desco_hip.h ("COLOUR REFINEMENT").  ``hash_refine``: that definition's hash chain restated with Python integers.
"""
import functools

import numpy as np

MASK = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


def mix(x):
    x &= MASK
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK
    x ^= x >> 31
    return x


def signed(x):
    return x - (1 << 64) if x >> 63 else x


def _segments(seg_ptr, anchor_base):
    for i in range(len(seg_ptr) - 1):
        rows = list(range(int(seg_ptr[i]), int(seg_ptr[i + 1])))
        yield i, rows, (int(anchor_base) + i if anchor_base >= 0 else None)


def _entries(vrowptr, vcol, slots, r, s):
    return vcol[vrowptr[r * slots + s]:vrowptr[r * slots + s + 1]]


def _lists(vrowptr, vcol):
    return [int(x) for x in vrowptr], [int(x) for x in vcol]


def hash_refine(vrowptr, vcol, num_rows, slots, group, seg_ptr, anchor_base, rounds, init=None):
    """(sig [S], colours [R], status [S]) as Python lists of signed 64-bit integers; a guarded segment has status -1 and
    None for its signature (its rows' colours stay None)."""
    vrowptr, vcol = _lists(vrowptr, vcol)
    sig, status, colours = [], [], [None] * num_rows
    for i, rows, a in _segments(seg_ptr, anchor_base):
        mine = rows + ([a] if a is not None else [])
        member = set(mine)
        if any(c not in member for r in mine for s in range(slots) for c in _entries(vrowptr, vcol, slots, r, s)):
            sig.append(None), status.append(-1)
            continue
        c = {r: (int(init[r]) & MASK) if init is not None else int(r == a) for r in mine}
        for _ in range(rounds):
            new = {}
            for r in mine:
                m = [0] * slots
                for s in range(slots):
                    for src in _entries(vrowptr, vcol, slots, r, s):
                        m[group[s]] = (m[group[s]] + mix(c[src] + G)) & MASK
                h = mix(c[r] + G)
                for g in range(slots):
                    h = mix(h ^ ((m[g] + (g + 1) * G) & MASK))
                new[r] = h
            c = new
        p = sum(mix(c[r] + G) for r in rows) & MASK
        sig.append(signed(mix(mix(c[a] + G) ^ ((p + G) & MASK)) if a is not None else mix(p + G)))
        status.append(0)
        for r in mine:
            colours[r] = signed(c[r])
    return sig, colours, status


def exact_refine(vrowptr, vcol, num_rows, slots, group, seg_ptr, anchor_base, rounds, init=None):
    """One hashable exact signature per segment: equal iff the segments agree under ``rounds`` rounds of refinement."""
    vrowptr, vcol = _lists(vrowptr, vcol)
    segs = [(rows, a) for _, rows, a in _segments(seg_ptr, anchor_base)]
    c = {}
    for rows, a in segs:
        for r in rows + ([a] if a is not None else []):
            c[r] = int(init[r]) if init is not None else int(r == a)
    ngroups = slots
    for _ in range(rounds):
        intern, new = {}, {}
        for r in c:
            ms = [[] for _ in range(ngroups)]
            for s in range(slots):
                ms[group[s]].extend(c[src] for src in _entries(vrowptr, vcol, slots, r, s))
            key = (c[r],) + tuple(tuple(sorted(m)) for m in ms)
            new[r] = intern.setdefault(key, len(intern))
        c = new
    return [(None if a is None else c[a], tuple(sorted(c[r] for r in rows))) for rows, a in segs]


def partition_of(labels):
    """The partition that equal labels induce, as a canonical list: the members of every class, classes by first member"""
    classes = {}
    for i, x in enumerate(labels):
        classes.setdefault(x if not isinstance(x, np.generic) else x.item(), []).append(i)
    return sorted(classes.values())


def refines(fine, coarse):
    """every class of ``fine`` lies inside one class of ``coarse``"""
    seen = {}
    return all(seen.setdefault(f if not isinstance(f, np.generic) else f.item(), c) == c for f, c in zip(fine, coarse))


@functools.lru_cache(maxsize=None)
def atlas_connected():
    """[(n, edges)]: the 994 connected graphs of 3..7 nodes of the networkx atlas, in atlas order"""
    import networkx as nx
    from networkx.generators.atlas import graph_atlas_g
    out = [(g.number_of_nodes(), sorted((min(a, b), max(a, b)) for a, b in g.edges()))
           for g in graph_atlas_g() if 3 <= g.number_of_nodes() <= 7 and nx.is_connected(g)]
    assert len(out) == 994
    return out


def anchored_at_largest(graph, anchor):
    """``graph`` relabelled so that ``anchor`` is its largest id (the two ids are exchanged)"""
    n, edges = graph
    swap = {anchor: n - 1, n - 1: anchor}
    return n, sorted((min(swap.get(a, a), swap.get(b, b)), max(swap.get(a, a), swap.get(b, b))) for a, b in edges)


def triangles(graph):
    n, edges = graph
    adj = [set() for _ in range(n)]
    for a, b in edges:
        adj[a].add(b), adj[b].add(a)
    return sum(len(adj[a] & adj[b]) for a, b in edges) // 3


# the pairs of the issue, as positions in ``atlas_connected()``: (graph, anchor) twice
PAIR_PLAIN_BLIND = ((250, 6), (251, 6))         # 0 / 2 triangles: merged under "plain", split under "shmp"
PAIR_SHMP_BLIND = ((753, 6), (754, 4))          # wheel W6 at its hub (6 triangles) / an apex over two triangles (8)
PAIR_GRAPHS_PLAIN_BLIND = (64, 66)              # whole graphs, 0 / 2 triangles: merged under "plain"


# ---- the inputs both test files run (built once per process) ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def graph_sets():
    """{name: GraphSet}: the atlas, the golden graphs, a 64-graph cox2-shaped slice and a small slice of a thinned
    syn_1827-shaped schedule"""
    from helpers import golden_graphs
    from desco_amd import synthetic
    from desco_amd.graphs import GraphSet
    return {"atlas": GraphSet.from_edge_lists(atlas_connected()),
            "golden": GraphSet.from_edge_lists(golden_graphs(max_n=40)),
            "cox2": synthetic.cox2_shaped().subset(0, 64),
            "syn": synthetic.syn_1827_shaped(60).subset(2, 8)}          # 6 graphs of the schedule's small end


@functools.lru_cache(maxsize=None)
def blocks():
    """{name: (Block of numpy arrays, the views defined on it)}: every graph set as whole graphs ("<set>/graphs") and as
    canonical neighborhoods of depth 4 under both definitions ("<set>/ball", "<set>/restricted")"""
    from desco_amd import expressiveness as X
    from desco_amd.batch import GraphBatch
    from desco_amd.partition import build_partition
    out = {}
    for name, g in graph_sets().items():
        b = X._block(GraphBatch(g, "cpu"))
        out[name + "/graphs"] = (X.Block(b.vrowptr.numpy(), b.vcol.numpy(), b.num_rows, 2, b.seg_ptr.numpy(), -1),
                                 ("plain", "shmp"))
        for restricted in (False, True):
            out[name + ("/restricted" if restricted else "/ball")] = (
                X._block(build_partition(g, 4, restricted=restricted)), ("plain", "hetero", "shmp"))
    return out


def block_args(b, group):
    """the positional arguments of ``hash_refine`` / ``exact_refine`` up to ``rounds``"""
    return (b.vrowptr, b.vcol, b.num_rows, b.slots, group, b.seg_ptr, b.anchor_base)
