"""Plain Python evaluation of the generator definition of include/desco_hip.h, "GRAPH GENERATORS": its own Philox, sets
for adjacency, nothing shared with the library.  ``generate`` returns what the twin and the kernel have to return bit
for bit; ``body`` stops before connection and relabel (the distribution tests compare that with networkx)."""
import numpy as np

M32 = 0xFFFFFFFF
ER, WS, RANDOM, BA, EBA, POWER = range(6)
BODY, RANDOM_BODY, CONNECT, RELABEL, WS_TRY = 0, 1, 2, 3, 16
FELL_BACK = 101


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def word(seed, graph, stream, i):
    t = i >> 2
    return philox4x32_10((t & M32, t >> 32, graph & M32, stream), (seed & M32, seed >> 32))[i & 3]


class Rng:
    def __init__(self, seed, graph, stream):
        self.seed, self.graph, self.stream, self.i, self.buf = seed, graph, stream, 0, None

    def next(self):
        if self.i & 3 == 0:
            t = self.i >> 2
            self.buf = philox4x32_10((t & M32, t >> 32, self.graph & M32, self.stream),
                                     (self.seed & M32, self.seed >> 32))
        self.i += 1
        return self.buf[(self.i - 1) & 3]

    def below(self, w):
        return (self.next() * w) >> 32


class Graph:
    def __init__(self, n):
        self.n, self.adj = n, [set() for _ in range(n)]

    def has(self, u, v):
        return v in self.adj[u]

    def add(self, u, v):
        self.adj[u].add(v), self.adj[v].add(u)

    def remove(self, u, v):
        self.adj[u].remove(v), self.adj[v].remove(u)

    def deg(self, v):
        return len(self.adj[v])

    def edges(self):
        return sorted((u, v) for u in range(self.n) for v in self.adj[u] if u < v)

    def num_edges(self):
        return sum(len(a) for a in self.adj) // 2


def choose(weights, r):
    """the node whose interval of the prefix weights holds r"""
    acc = 0
    for v, w in enumerate(weights):
        acc += w
        if r < acc:
            return v
    raise AssertionError("r is not below the total weight")


def distinct(rng, weights, m):
    total, out = sum(weights), []
    while len(out) < m:
        x = choose(weights, rng.below(total))
        if x not in out:
            out.append(x)
    return out


def er_body(g, seed, graph, thr):
    for v in range(1, g.n):
        for u in range(v):
            if word(seed, graph, BODY, v * (v - 1) // 2 + u) < thr:
                g.add(u, v)


def random_body(g, seed, graph, m):
    n = g.n
    if m >= n * (n - 1) // 2:
        for v in range(n):
            for u in range(v):
                g.add(u, v)
        return
    rng, e = Rng(seed, graph, RANDOM_BODY), 0
    while e < m:
        u, v = rng.below(n), rng.below(n)
        if u == v or g.has(u, v):
            continue
        g.add(u, v)
        e += 1


def ws_try(n, seed, graph, attempt, h, thr):
    g = Graph(n)
    for j in range(1, h + 1):
        for u in range(n):
            g.add(u, (u + j) % n)
    rng = Rng(seed, graph, WS_TRY + attempt)
    for j in range(1, h + 1):
        for u in range(n):
            if not rng.next() < thr:
                continue
            if g.deg(u) >= n - 1:
                continue
            w = rng.below(n)
            while w == u or g.has(u, w):
                w = rng.below(n)
            g.remove(u, (u + j) % n)
            g.add(u, w)
    return g


def ba_body(g, seed, graph, m):
    for v in range(1, m + 1):
        g.add(0, v)
    rng = Rng(seed, graph, BODY)
    for s in range(m + 1, g.n):
        for x in distinct(rng, [g.deg(v) for v in range(s)], m):
            g.add(s, x)


def eba_body(g, seed, graph, m, t_add, t_rewire):
    rng = Rng(seed, graph, BODY)
    for s in range(m, g.n):
        full, edges = s - 1, g.num_edges()
        room = s * full // 2

        def around(x):
            return [0 if v == x or g.has(x, v) else g.deg(v) + 1 for v in range(s)]

        a = rng.next()
        if a < t_add:
            if edges + m <= room:
                flagged = [v for v in range(s) if g.deg(v) < full]
                for _ in range(m):
                    if not flagged:
                        break
                    src = flagged[rng.below(len(flagged))]
                    w = around(src)
                    if sum(w) == 0:
                        break
                    dst = choose(w, rng.below(sum(w)))
                    g.add(src, dst)
                    if g.deg(src) == full:
                        flagged.remove(src)
                    if g.deg(dst) == full and dst in flagged:
                        flagged.remove(dst)
        elif a < t_rewire:
            if m <= edges < room:
                flagged = [v for v in range(s) if 0 < g.deg(v) < full]
                for _ in range(m):
                    if not flagged:
                        break
                    node = flagged[rng.below(len(flagged))]
                    if g.deg(node) == 0:
                        break
                    old = sorted(g.adj[node])[rng.below(g.deg(node))]
                    w = around(node)
                    if sum(w) == 0:
                        break
                    dst = choose(w, rng.below(sum(w)))
                    g.remove(node, old)
                    g.add(node, dst)
                    if g.deg(old) == 0 and old in flagged:
                        flagged.remove(old)
                    if dst in flagged:
                        if g.deg(dst) == full:
                            flagged.remove(dst)
                    elif g.deg(dst) == 1:
                        flagged.append(dst)
                        flagged.sort()                  # (the k-th flagged node in id order)
        for x in distinct(rng, [g.deg(v) + 1 for v in range(s)], m):
            g.add(s, x)


def power_body(g, seed, graph, m, thr):
    rng = Rng(seed, graph, BODY)
    weight = [1] * m + [0] * (g.n - m)
    for s in range(m, g.n):
        targets = distinct(rng, weight[:s], m)
        target = targets.pop(0)
        g.add(s, target)
        weight[target] += 1
        count = 1
        while count < m:
            if rng.next() < thr:
                near = sorted(x for x in g.adj[target] if x != s and not g.has(s, x))
                if near:
                    x = near[rng.below(len(near))]
                    g.add(s, x)
                    weight[x] += 1
                    continue
            target = targets.pop(0)
            g.add(s, target)
            weight[target] += 1
            count += 1
        weight[s] += m


def component_labels(g):
    label = [-1] * g.n
    for s in range(g.n):
        if label[s] >= 0:
            continue
        label[s], stack = s, [s]
        while stack:
            v = stack.pop()
            for u in g.adj[v]:
                if label[u] < 0:
                    label[u] = s
                    stack.append(u)
    return label


def pruefer_tree(seq, c):
    """the edges (leaf, entry) of the labelled tree on c >= 2 nodes, the smallest leaf first"""
    degree = [1] * c
    for x in seq:
        degree[x] += 1
    edges = []
    for x in seq:
        leaf = min(v for v in range(c) if degree[v] == 1)
        edges.append((leaf, x))
        degree[leaf], degree[x] = 0, degree[x] - 1
    leaf = min(v for v in range(c) if degree[v] == 1)
    edges.append((leaf, c - 1))
    return edges


def connect(g, seed, graph):
    label = component_labels(g)
    roots = sorted(set(label))
    c = len(roots)
    if c <= 1:
        return 0
    members = [[v for v in range(g.n) if label[v] == r] for r in roots]
    rng = Rng(seed, graph, CONNECT)
    seq = [rng.below(c) for _ in range(c - 2)]
    for i, j in pruefer_tree(seq, c):
        a = members[i][rng.below(len(members[i]))]
        b = members[j][rng.below(len(members[j]))]
        g.add(a, b)
    return c - 1


def body(family, n, a, b, t0, t1, seed, graph):
    """(graph before connection and relabel, WS tries)"""
    g, tries = Graph(n), 0
    if n == 1:
        return g, 0
    if family == ER:
        er_body(g, seed, graph, t0)
    elif family == RANDOM:
        random_body(g, seed, graph, a)
    elif family == BA:
        ba_body(g, seed, graph, a)
    elif family == EBA:
        eba_body(g, seed, graph, a, t0, t1)
    elif family == POWER:
        power_body(g, seed, graph, a, t0)
    else:
        h, tries = a // 2, FELL_BACK
        for attempt in range(100 if h > 0 else 0):
            t = ws_try(n, seed, graph, attempt, h, t0)
            if len(set(component_labels(t))) == 1:
                g, tries = t, attempt + 1
                break
        if tries == FELL_BACK:
            random_body(g, seed, graph, b)
    return g, tries


def generate_one(family, n, a, b, t0, t1, seed, graph):
    """(rows of new ids: list of ascending neighbour lists, status word)"""
    g, tries = body(family, n, a, b, t0, t1, seed, graph)
    added = connect(g, seed, graph)
    order = sorted(range(n), key=lambda v: (word(seed, graph, RELABEL, v), v))
    rank = [0] * n
    for i, v in enumerate(order):
        rank[v] = i
    rows = [sorted(rank[u] for u in g.adj[v]) for v in order]
    return rows, tries | (added << 8)


def generate(family, n, param, threshold, seed=0, graph_base=0):
    """(graph_ptr, rowptr, col, deg, status) as numpy arrays, the layout of ``generators.Generated``"""
    graph_ptr, rowptr, col, status = [0], [0], [], []
    for g in range(len(n)):
        rows, st = generate_one(int(family[g]), int(n[g]), int(param[g][0]), int(param[g][1]), int(threshold[g][0]),
                                int(threshold[g][1]), seed, graph_base + g)
        for r in rows:
            col.extend(graph_ptr[-1] + u for u in r)
            rowptr.append(len(col))
        graph_ptr.append(graph_ptr[-1] + int(n[g]))
        status.append(st)
    return (np.array(graph_ptr, np.int64), np.array(rowptr, np.int64), np.array(col, np.int32),
            np.diff(np.array(rowptr, np.int64)).astype(np.int32), np.array(status, np.int32))
