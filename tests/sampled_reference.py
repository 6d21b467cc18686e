"""A pure Python / numpy restatement of the sampled counts (include/desco_hip.h, "SAMPLED COUNTS"), written from the
header's text: the key-ordered enumeration tree, the decision chain, the tallies.  For graphs of a few dozen nodes."""
import functools
import itertools

import numpy as np

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
G = 0x9E3779B97F4A7C15
TAG = 0x53414D50


def mix(x):
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    x ^= x >> 31
    return x


def philox4x32_10(c, k):
    c0, c1, c2, c3 = c
    k0, k1 = k
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def root_hash(seed, graph, replica, s0):
    w = philox4x32_10((s0, graph & M32, replica & M32, TAG), (seed & M32, (seed >> 32) & M32))
    return w[0] | w[1] << 32


def step(h, u):
    return mix(h ^ ((u + 1) * G & M64))


def pair_bit(a, b):
    a, b = min(a, b), max(a, b)
    return b * (b - 1) // 2 + a


@functools.lru_cache(maxsize=None)
def canonical(k, mask):
    """the smallest mask among the relabelings of the k-node adjacency mask"""
    pairs = [(a, b) for b in range(1, k) for a in range(b) if mask >> pair_bit(a, b) & 1]
    return min(sum(1 << pair_bit(p[a], p[b]) for a, b in pairs) for p in itertools.permutations(range(k)))


def query_key(n, edges):
    return n, canonical(n, sum(1 << pair_bit(a, b) for a, b in set((min(a, b), max(a, b)) for a, b in edges)))


def tallies(graphs, queries, thr, replicas, seed=0, graph_base=0, replica_base=0):
    """graphs: [(n, edges)], queries: [(k, edges)] pairwise non-isomorphic; thr: integers, thr[d] for d = 2..kmax.
    Returns int64 [replicas, total nodes, len(queries)]."""
    kmax = len(thr) - 1
    column = {query_key(k, e): q for q, (k, e) in enumerate(queries)}
    total = sum(n for n, _ in graphs)
    out = np.zeros((replicas, total, len(queries)), dtype=np.int64)
    base = 0
    for gi, (n, edges) in enumerate(graphs):
        rows = [[] for _ in range(n)]
        for a, b in set((min(a, b), max(a, b)) for a, b in edges):
            rows[a].append(b)
            rows[b].append(a)
        rows = [sorted(r) for r in rows]
        adj = [set(r) for r in rows]
        for r in range(replicas):

            def extend(S, mask, h, key, v):
                # the children of the sequence S: candidates behind `key` = (index of the first adjacent member,
                # position in that member's row), in key order
                j = len(S)
                for i in range(key[0], j):
                    for pos in range(key[1] if i == key[0] else 0, len(rows[S[i]])):
                        u = rows[S[i]][pos]
                        if u >= v:
                            break
                        if u in S or any(u in adj[S[t]] for t in range(i)):
                            continue                    # a member, or its first adjacent member comes before S[i]
                        h2 = step(h, u)
                        if not (h2 >> 32) < thr[j + 1]:
                            continue                    # dropped, with everything below it
                        m2 = mask | sum(1 << pair_bit(t, j) for t in range(j) if u in adj[S[t]])
                        q = column.get((j + 1, canonical(j + 1, m2)))
                        if q is not None:
                            out[r, base + v, q] += 1
                        if j + 1 < kmax:
                            extend(S + [u], m2, h2, (i, pos + 1), v)

            for v in range(n):
                extend([v], 0, root_hash(seed, graph_base + gi, replica_base + r, v), (0, 0), v)
        base += n
    return out
