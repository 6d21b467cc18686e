"""Host reference of the fused gossip stage (include/desco_hip.h, "Fused gossip stage"; header of csrc/gossip_f16.hip),
written from the documented contract alone: numpy + torch, ``index_add_`` over an explicit edge list, no call into
``oracle/`` or ``desco_amd``.  Used by tests/test_gossip_kernels_gpu.py (the kernels against it) and by
tests/test_gossip_reference_host.py (the reference against a dense-matrix formula, and the gate against a second fp32
summation order).

    a_l = g_l[q] deg_lo(i) + (1 - g_l[q]) deg_hi(i)      b0 = g0[q] sum_{j<i} x[j,q] + (1 - g0[q]) sum_{j>i} x[j,q]
    h1 = relu(a0 p_q + b0 r + x t + z_q)                 hh = sum_j (j<i ? g1 : 1 - g1) h1_j
    h2 = relu([hh|h1] W1^T + a1 u + d1)                  y1 = leaky_0.1([h1|h2] Wp^T + x tp + zp_q)
    y2 = relu(y1 W3^T + b3)    y3 = relu(y2 W5^T + b5)   out = x + b7 + sum_c y3[c] w7[c]

``scalars`` evaluates the first line (the records (a0, b0, a1, x) of desco_gossip_scalars_f32), ``net`` the rest from
such records, each in the dtype asked for: float64 is the reference, float32 the *fp32 evaluation* the kernels are held
to.  ``net`` also returns D[i,q] = |x| + |b7| + sum_c |y3[c] w7[c]|, the sum of absolute terms of the last dot product:
the scale the output's rounding errors live on."""
import numpy as np
import torch


# ---- graphs ---------------------------------------------------------------------------------------------------------
class Graph:
    """Symmetric graph on ids 0..n-1: directed edge list (src = row, dst = neighbour, dst ascending within a row) and the
    CSR the kernels take.  ``col`` is never empty (a graph without edges gets one unused entry: a valid pointer)."""

    def __init__(self, n, edges):
        und = {(min(a, b), max(a, b)) for a, b in edges if a != b}
        assert all(0 <= a and b < n for a, b in und)
        src = np.array([a for a, b in und] + [b for a, b in und], dtype=np.int64)
        dst = np.array([b for a, b in und] + [a for a, b in und], dtype=np.int64)
        o = np.lexsort((dst, src))
        self.n = int(n)
        self.edges = sorted(und)
        self.src, self.dst = torch.from_numpy(src[o]), torch.from_numpy(dst[o])
        self.deg = np.bincount(src, minlength=n).astype(np.int64)
        self.rowptr = np.concatenate([[0], np.cumsum(self.deg)]).astype(np.int32)
        self.col = dst[o].astype(np.int32) if len(o) else np.zeros(1, np.int32)


def ladder_edges():
    """Disjoint cliques K_1 .. K_18, K_32, K_34 on consecutive ids: d + 1 consecutive nodes of degree exactly d for
    d = 0..17, 31, 33, the inner nodes of a clique with neighbours on both sides of their id (237 nodes)."""
    edges, n = [], 0
    for k in list(range(1, 19)) + [32, 34]:
        edges += [(n + a, n + b) for a in range(k) for b in range(a + 1, k)]
        n += k
    return n, edges


def permuted(n, edges, seed):
    perm = np.random.default_rng(seed).permutation(n)
    return n, [(int(perm[a]), int(perm[b])) for a, b in edges]


def prefix(n_keep, edges):
    """the first n_keep ids with the edges among them (a prefix of a graph, re-closed)"""
    return n_keep, [(a, b) for a, b in edges if a < n_keep and b < n_keep]


STAR_LEAVES = 1300      # more than one staging pass of the bf16x6 kernel (gossip_fused.hip: ECAP = PCAP = 1216 records)


def hub_edges():
    """A set of 2000 ids made of three parts.  (a) 1700 ids: a star whose centre (id 850) has STAR_LEAVES leaves spread
    over the whole id range, the other ~400 ids isolated, so that the centre's wave group holds one long row among
    rows of degree 0 and 1.  (b) 60 ids: the last adjacent to every lower id, the first to every higher one.  (c) 240
    ids, all isolated but one node with 40 neighbours on both sides."""
    n, centre = 1700, 850
    others = [v for v in range(n) if v != centre]
    step = len(others) / STAR_LEAVES
    leaves = sorted({others[int(i * step)] for i in range(STAR_LEAVES)})
    assert len(leaves) == STAR_LEAVES
    star = (n, [(centre, v) for v in leaves])
    fan = (60, [(v, 59) for v in range(59)] + [(0, v) for v in range(1, 59)])
    lone = (240, [(100, v) for v in list(range(60, 80)) + list(range(150, 170))])
    return concat([star, fan, lone])


def concat(graphs):
    """disjoint union, ids shifted: [(n, edges), ...] -> (n, edges)"""
    n, edges = 0, []
    for m, e in graphs:
        edges += [(a + n, b + n) for a, b in e]
        n += m
    return n, edges


# ---- the property the fused kernels rely on in desco_gossip_tile_order's output ---------------------------------------
def check_tile_order(perm, rowptr, num_nodes):
    """perm: uint8 values [tiles * 128] as desco_gossip_tile_order wrote them.  Every 128-node tile holds a permutation
    of 0..127; sorted rank s (rows by decreasing degree, ties -- the padded slots of a ragged last tile count as degree
    0 -- in node order, so padded slots come last) sits at slot 16 w + 2 g + (s & 1) with pair = s >> 1, g = pair >> 3
    and w = the pair's snake position (pair & 7, reversed for odd g)."""
    perm = np.asarray(perm).astype(np.int64).reshape(-1, 128)
    tiles = (num_nodes + 127) // 128
    assert perm.shape[0] == tiles
    assert (np.sort(perm, axis=1) == np.arange(128)).all(), "every tile must hold a permutation of 0..127"
    deg = np.zeros(tiles * 128, np.int64)
    deg[:num_nodes] = np.diff(np.asarray(rowptr).astype(np.int64))[:num_nodes]
    for t in range(tiles):
        d = deg[128 * t + perm[t]].reshape(8, 8, 2)            # [wave][pair][half]
        pair_cost = d.max(2)                                    # lock-stepped halves
        order = np.concatenate([pair_cost[:, g] if g % 2 == 0 else pair_cost[::-1, g] for g in range(8)])
        assert (np.diff(order) <= 0).all(), "pairs must be dealt in snake order of decreasing cost"
        assert (d[:, :, 0] >= d[:, :, 1]).all()
        ranks = np.argsort(-deg[128 * t:128 * (t + 1)], kind="stable")      # ties in node order, padded slots last
        want = np.empty(128, np.int64)
        for s, row in enumerate(ranks):
            pair = s >> 1
            g, slot = pair >> 3, pair & 7
            want[16 * (7 - slot if g & 1 else slot) + 2 * g + (s & 1)] = row
        assert (perm[t] == want).all(), f"tile {t}: not the stable degree order"
        pad = np.arange(128)[128 * t + np.arange(128) >= num_nodes]
        if len(pad):
            assert set(ranks[128 - len(pad):]) == set(pad), "padded slots must be sorted last"


# ---- operands -------------------------------------------------------------------------------------------------------
REGIMES = ("o1", "x1e6", "x1e-3", "rows2^18", "wscales", "halfzero", "deadrelu", "g1exact")


def operands(Q, regime, seed):
    """The operand set of one case, fp32 on the host: gates g0, g1 [Q]; p, z, zp [Q, 64]; r, t, u, tp, d1, b3 [64];
    b5, w7 [256]; the fp32 weight matrices w1, wp [64, 128], w3 [64, 64], w5 [256, 64] ([out, in]); b7 (float)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                       # noqa: E731
    P = dict(g0=torch.rand(Q, generator=g), g1=torch.rand(Q, generator=g), p=0.3 * r(Q, 64), z=0.5 * r(Q, 64),
             zp=0.5 * r(Q, 64), r=0.1 * r(64), t=0.2 * r(64), u=0.2 * r(64), tp=0.2 * r(64), d1=0.3 * r(64),
             w1=r(64, 128) / np.sqrt(128), wp=r(64, 128) / np.sqrt(128), w3=r(64, 64) / 8, b3=0.3 * r(64),
             w5=r(256, 64) / 8, b5=0.3 * r(256), w7=r(256) / 16, b7=0.1)
    if regime == "wscales":
        # weights x3, the four matrices at four scales 2^8 apart (1 / scale of their fp16 planes differs likewise), in
        # an order that keeps every stage's signal above its bias: gains 2^4, 1, 2^12, 1 after the four matrices
        for k, e in (("w1", 4), ("wp", -4), ("w3", 12), ("w5", -12)):
            P[k] = P[k] * (3.0 * 2.0 ** e)
    elif regime == "deadrelu":
        # z_q and d1 shifted negative: h1 (and with it hh, then h2) of low-degree nodes with small x is exactly zero
        P["z"] = P["z"] - 4.0
        P["d1"] = P["d1"] - 6.0
    elif regime == "g1exact":
        P["g1"][0::3] = 0.0
        P["g1"][1::3] = 1.0
    elif regime == "zeros":
        for k in ("p", "z", "zp", "r", "t", "u", "tp", "d1", "b3", "b5"):
            P[k] = torch.zeros_like(P[k])
    return P


def features(N, Q, regime, seed):
    """x [N, Q] fp32 (the neighbourhood counts a gossip pass corrects) of one case"""
    rng = np.random.default_rng(seed + 1000)
    g = torch.Generator().manual_seed(seed + 2000)
    x = torch.from_numpy(rng.gamma(1.0, 4.0, size=(N, Q))).float()
    if regime == "x1e6":
        x = torch.rand(N, Q, generator=g) * 1e6
    elif regime == "x1e-3":
        x = torch.rand(N, Q, generator=g) * 1e-3
    elif regime == "rows2^18":
        x = torch.rand(N, Q, generator=g) * 2.0 ** torch.randint(-18, 19, (N, 1), generator=g).float()
    elif regime == "halfzero":
        x[torch.arange(N) % 2 == 1] = 0
    elif regime == "zeros":
        x = torch.zeros(N, Q)
    return x


# ---- the formulas ---------------------------------------------------------------------------------------------------
def scalars(x, G, g0, g1, dtype=torch.float64):
    """(scal4 [N, Q, 4] = (a0, b0, a1, x), mag [N, Q, 4] = the same formula on absolute values) in ``dtype``"""
    x, g0, g1 = x.to(dtype), g0.to(dtype), g1.to(dtype)
    N, Q = x.shape
    lo = G.dst < G.src
    one = torch.ones(len(G.src), dtype=dtype)
    dlo = torch.zeros(N, dtype=dtype).index_add_(0, G.src[lo], one[lo])[:, None]
    dhi = torch.zeros(N, dtype=dtype).index_add_(0, G.src[~lo], one[~lo])[:, None]

    def b0(v):
        slo = torch.zeros(N, Q, dtype=dtype).index_add_(0, G.src[lo], v[G.dst[lo]])
        shi = torch.zeros(N, Q, dtype=dtype).index_add_(0, G.src[~lo], v[G.dst[~lo]])
        return g0 * slo + (1 - g0) * shi                       # (gates lie in [0, 1]: they are their own absolute values)

    a0 = g0 * dlo + (1 - g0) * dhi
    a1 = g1 * dlo + (1 - g1) * dhi
    scal = torch.stack([a0, b0(x), a1, x], -1)
    mag = torch.stack([a0.abs(), b0(x.abs()), a1.abs(), x.abs()], -1)
    return scal, mag


def _mm(a, w, chunk):
    """a @ w^T: whole-K, or K in ``chunk``-wide pieces summed from the last piece to the first"""
    if chunk is None:
        return a @ w.t()
    acc = None
    for k in range(w.shape[1] - chunk, -1, -chunk):
        part = a[..., k:k + chunk] @ w[:, k:k + chunk].t()
        acc = part if acc is None else acc + part
    return acc


def net(scal4, G, P, dtype=torch.float64, chunk=None, row_budget=1 << 21):
    """From records scal4 [N, Q, 4] (any float dtype; taken as exact): (out [N, Q], D [N, Q], stats) in ``dtype``.
    stats: fractions of (node, query) rows whose whole h1 / h2 vector is zero.  Queries are independent and are taken
    in blocks so that no intermediate exceeds ``row_budget`` rows of 256 values."""
    c = lambda v: v.to(dtype)                                                         # noqa: E731
    N, Q = scal4.shape[:2]
    src, dst = G.src, G.dst
    lo = dst < src
    qb = max(1, min(Q, row_budget // max(N, len(src), 1)))
    outs, Ds, z1, z2 = [], [], 0, 0
    r, t, u, tp, d1, b3, b5, w7 = (c(P[k]) for k in ("r", "t", "u", "tp", "d1", "b3", "b5", "w7"))
    w1, wp, w3, w5 = (c(P[k]) for k in ("w1", "wp", "w3", "w5"))
    b7 = torch.tensor(P["b7"], dtype=torch.float32).to(dtype)
    for q0 in range(0, Q, qb):
        s = c(scal4[:, q0:q0 + qb])
        a0, b0, a1, x = s[..., 0, None], s[..., 1, None], s[..., 2, None], s[..., 3, None]
        g1, p, z, zp = (c(P[k][q0:q0 + qb]) for k in ("g1", "p", "z", "zp"))
        h1 = torch.relu(a0 * p + b0 * r + x * t + z)                                  # [N, qb, 64]
        gate = torch.where(lo[:, None], g1[None, :], 1 - g1[None, :])                 # [E, qb]
        hh = torch.zeros_like(h1).index_add_(0, src, gate[..., None] * h1[dst])
        h2 = torch.relu(_mm(torch.cat([hh, h1], -1), w1, chunk) + a1 * u + d1)
        y1 = torch.nn.functional.leaky_relu(_mm(torch.cat([h1, h2], -1), wp, chunk) + x * tp + zp, 0.1)
        y2 = torch.relu(_mm(y1, w3, chunk) + b3)
        y3 = torch.relu(_mm(y2, w5, chunk) + b5)
        terms = y3 * w7
        outs.append(x[..., 0] + b7 + terms.sum(-1))
        Ds.append(x[..., 0].abs() + b7.abs() + terms.abs().sum(-1))
        z1 += int((h1 == 0).all(-1).sum())
        z2 += int((h2 == 0).all(-1).sum())
    stats = {"h1_zero": z1 / max(N * Q, 1), "h2_zero": z2 / max(N * Q, 1)}
    return torch.cat(outs, 1), torch.cat(Ds, 1), stats


def scaled_error(got, ref, D):
    """(E = max |got - ref| / D over the elements, flat index of the worst one); an exact element counts 0 whatever D"""
    err = (got.double() - ref).abs()
    e = torch.where(err == 0, torch.zeros_like(err), err / D)
    e = torch.nan_to_num(e, nan=float("inf"))
    i = int(e.flatten().argmax()) if e.numel() else 0
    return (float(e.flatten()[i]) if e.numel() else 0.0), i
