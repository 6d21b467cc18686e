"""Host reference of the gossip training trunks (the docstrings of autograd.GossipTrunk / GossipTrunkDeep; DESIGN.md
4.2) at the trunk's operand level, written from that contract alone: numpy + torch, ``index_add_`` over an explicit edge
list, forward AND backward written out, no call into ``desco_amd.ops``, ``desco_amd.autograd`` or ``oracle/``.  Used by
tests/test_gossip_trunk_kernels_gpu.py (the three backward forms against it) and by
tests/test_gossip_trunk_reference_host.py (the reference against a dense-matrix formula and torch autograd, the gate
against a second fp32 summation order, and known chain errors against the gate).

With r = i Q + q and f_1 .. f_L, f_p the dropout factors (0 or 1 / (1 - p)) or 1:

    h_1     = f_1 relu(C6[r] . V0[q])
    hh_l    = sum_j (j < i ? g_l[q] : 1 - g_l[q]) h_l[j, q]
    h_{l+1} = f_{l+1} relu([hh_l | h_l] wt_l + C3[r] . V_l[q])                 l = 1 .. L - 1
    y       = f_p leaky_0.1([h_1 | .. | h_L] wtp + C2[r] . Vp[q])
    y3 = relu(y w3t + b3)     y5 = relu(y3 w5t + b5)     pred = x + b7 + y5 . w7

    C6 = (deg_hi, deg_lo - deg_hi, s_hi, s_lo - s_hi, x, 1)   C3 = (deg_hi, deg_lo - deg_hi, 1)   C2 = (x, 1)
    deg_lo(i) = #{j ~ i, j < i}, s_lo(i, q) = sum_{j ~ i, j < i} x[j, q]; _hi: j > i   (gnn_model.gossip_forward_train)

A *case* is a dict: G (gossip_reference.Graph), N, Q, L, x [N, Q], C6 / C3 / C2, the operands V0 [Q, 6, 64], g / wt / V
(lists of L - 1: [Q], [128, 64], [Q, 3, 64]), wtp [64 L, 64], Vp [Q, 2, 64], w3t [64, 64], b3, w5t [64, 256], b5, w7 [256],
b7 [1], dpred [R] -- all fp32 -- and ``factors``: None or {"h1": [R, 64], .., "post": [R, 64]}.

``evaluate`` returns every activation (h{l}, hh{l}, y, y3, y5, pred) and every gradient the nodes return (dV0, dg{l},
dwt{l}, dV{l}, dwtp, dVp, dw3t, db3, dw5t, db5, dw7, db7) in the dtype asked for: float64 is the reference, float32
the *fp32 evaluation* the kernels are held to, ``chunk`` a second fp32 summation order (K in ``chunk``-wide pieces and
rows in pieces of 8 ``chunk``, both summed from the last piece to the first, the edge list walked backwards).  With
``pins`` (a dict of activations h{l}, y, y3, y5 the caller supplies) relu' and leaky' come from them -- ``c > 0``, the
library's act'(c) on the activation OUTPUT (csrc/common_device.hpp apply_act, the gate of gemm_f32.hip) -- in the forward
and in the backward.  ``mag`` is the same function on the absolute values of every operand with pins and factors kept,
unpinned activations replaced by identity and the two signed parts of d/dg both taken positive: the sum of |terms| of
each element, the scale its rounding errors live on.  ``mutate`` evaluates a known chain error (MUTATIONS)."""
import collections
import functools

import numpy as np
import torch

from gossip_reference import Graph, concat, hub_edges, ladder_edges, permuted, prefix  # noqa: F401

H = 64
DEAD_COLS = slice(16, 32)               # the dead-relu regime's columns of h1, y3 (b3) and y5 (b5)
ZERO_Q = 2                              # the x1e6 regime's query column with x == 0
DROPS = ((0.3, 0.1), (0.0, 0.3))        # (p_layer, p_post): the two differ, so that neither can stand in for the other


# E_kernel <= FACTOR x E_f32.  4 is the project's gate.  dg_l (Q values, each a sum over all nodes of row dots) and db3
# (64 column sums over all rows) exceed it through the order of an fp32 sum alone: on so few elements the float32
# evaluation's own error is often a fraction of an ulp of the result, and the reduction orders of the kernels (row
# groups of 4 or 16 in one running sum each, ``_chains``) evaluated on the host, no kernel involved, reach 6.2x (dg) and
# 4.5x (db3) of it on the cases of ``CHAIN_EVIDENCE``.  Their factors are those host figures rounded up to an integer;
# tests/test_gossip_trunk_reference_host.py measures them again and holds the constants to the measurement.
FACTOR = collections.defaultdict(lambda: 4, dg=7, db3=5)
CHAIN_EVIDENCE = (("deep", "deep L9"), ("trunk", "ladder Q29"))


def family(k):
    """h_l, hh_l, dg_l, dwt_l, dV_l (l >= 1) are one family each; every other tensor is its own"""
    return k if k in ("y", "y3", "y5", "pred", "dV0", "dwtp", "dVp", "dw3t", "db3", "dw5t", "db5", "dw7", "db7") \
        else k.rstrip("0123456789")


def layer_site(l):
    """the documented dropout site ids (GossipTrunk.layer_site): h1 0, h2 1, post_mp.1 2, h_l l from 3 on"""
    return 0 if l == 1 else 1 if l == 2 else l


SITE_POST = 2


# ---- cases ----------------------------------------------------------------------------------------------------------
def constants(G, x, dtype=torch.float64):
    """(C6 [R, 6], C3 [R, 3], C2 [R, 2]) of a Graph and x [N, Q], evaluated in ``dtype``"""
    x = x.to(dtype)
    N, Q = x.shape
    lo = G.dst < G.src
    one = torch.ones(len(G.src), dtype=dtype)
    dlo = torch.zeros(N, dtype=dtype).index_add_(0, G.src[lo], one[lo])[:, None].expand(N, Q)
    dhi = torch.zeros(N, dtype=dtype).index_add_(0, G.src[~lo], one[~lo])[:, None].expand(N, Q)
    slo = torch.zeros(N, Q, dtype=dtype).index_add_(0, G.src[lo], x[G.dst[lo]])
    shi = torch.zeros(N, Q, dtype=dtype).index_add_(0, G.src[~lo], x[G.dst[~lo]])
    ones = torch.ones(N, Q, dtype=dtype)
    C6 = torch.stack([dhi, dlo - dhi, shi, slo - shi, x, ones], -1).reshape(N * Q, 6)
    C3 = torch.stack([dhi, dlo - dhi, ones], -1).reshape(N * Q, 3)
    C2 = torch.stack([x, ones], -1).reshape(N * Q, 2)
    return C6, C3, C2


def case(graph, Q, L, regime="o1", seed=0, weights="signed"):
    """One case: the constants from the graph and x in fp64 (rounded once to the fp32 operands every evaluation and
    the kernels share), every other operand and dpred random.  The per-query rows of V0 / V_l / Vp are scaled by the
    root mean square of their column of C over the nodes, and the gathered half of wt_l by that of the degrees, so
    that the activations of every layer are O(1) at any x and any depth.  Regimes:
    ``o1``        x = 20 rand.
    ``x1e6``      x up to 1e6 in the query columns q % 4 == 1 and exactly 0 in column ZERO_Q.
    ``g1exact``   every gate holds exact 0 (q % 3 == 0) and 1 (q % 3 == 1).
    ``deadrelu``  V0[:, 5], b3, b5 at -1e3 on DEAD_COLS: those columns of h1, y3, y5 are 0 on every row.
    ``weights="aligned"``: every weight matrix, w7, the non-constant rows of V and dpred non-negative, and the constant
    rows of V0 / V_l / Vp and b3 / b5 set to minus the median of their column's pre-activation (about half of every
    relu dead, half of y on the 0.1 branch).  With zero-mean weights the terms of a gradient cancel to 1e-4 .. 1e-8 of
    their absolute sum, and a chain error of the gradient's own size is that small on the scale ``mag``; aligned, a term
    counts for what it is (tests/test_gossip_trunk_reference_host.py measures both)."""
    n, edges = graph
    G = Graph(n, edges)
    N, R = G.n, G.n * Q
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)                                    # noqa: E731
    x = 20.0 * torch.rand(N, Q, generator=gen)
    if regime == "x1e6":
        x[:, 1::4] = 1e6 * torch.rand(N, len(range(1, Q, 4)), generator=gen)
        x[:, ZERO_Q] = 0.0
    C6, C3, C2 = (c.float() for c in constants(G, x))

    def per_query(C, amp):
        k = C.shape[1]
        rms = C.double().view(N, Q, k).pow(2).mean(0).sqrt().clamp_min(1.0).float()   # [Q, k]
        return amp * rn(Q, k, H) / rms[:, :, None]

    # the post_mp.0 block of h_l at its own scale 2 l / (L + 1) (mean 1): exchanged blocks differ by more than noise
    blocks = torch.repeat_interleave(2.0 * torch.arange(1, L + 1) / (L + 1), H)[:, None]
    dbar = max(1.0, float(np.sqrt((G.deg.astype(np.float64) ** 2).mean())))
    c = dict(G=G, N=N, Q=Q, L=L, R=R, regime=regime, x=x, C6=C6, C3=C3, C2=C2, factors=None,
             V0=per_query(C6, 0.5), Vp=per_query(C2, 0.3), wtp=rn(H * L, H) / np.sqrt(H * L) * blocks,
             g=[torch.rand(Q, generator=gen) for _ in range(L - 1)],
             wt=[torch.cat([rn(H, H) / (8.0 * dbar), rn(H, H) / 8.0]) * 1.2 for _ in range(L - 1)],
             V=[per_query(C3, 0.3) for _ in range(L - 1)],
             w3t=rn(H, H) / 8.0, b3=0.3 * rn(H), w5t=rn(H, 4 * H) / 8.0, b5=0.3 * rn(4 * H), w7=rn(4 * H) / 16.0,
             b7=torch.tensor([0.1]), dpred=rn(R))
    if regime == "g1exact":
        for g in c["g"]:
            g[0::3], g[1::3] = 0.0, 1.0
    elif regime == "deadrelu":
        c["V0"][:, 5, DEAD_COLS] = -1e3
        c["b3"][DEAD_COLS] = -1e3
        c["b5"][DEAD_COLS] = -1e3
    if weights == "aligned":
        _align(c)
    return c


def _align(c):
    """non-negative weights and seeds; stage by stage (fp64) each stage's weights are scaled to a pre-activation of
    unit spread and its constant term centres it"""
    N, Q, L = c["N"], c["Q"], c["L"]
    for k in ("V0", "Vp", "wtp", "w3t", "w5t", "w7", "dpred"):
        c[k] = c[k].abs()
    c["wt"], c["V"] = [w.abs() for w in c["wt"]], [v.abs() for v in c["V"]]
    aff = lambda C, Vq: torch.einsum("nqk,qkc->nqc", C.double().view(N, Q, -1), Vq.double())   # noqa: E731

    def centre(Vq, C, w, a):
        """w [K, 64] and Vq [Q, k, 64] scaled to unit spread of z = a w + C[:, :-1] . Vq[:, :-1] about its per-(query,
        column) median over the nodes, then the last (constant 1) row of Vq := - that median"""
        Vq[:, -1] = 0
        z = aff(C, Vq) + (0 if w is None else (a @ w.double()).view(N, Q, H))
        s = float((z - z.median(0).values).std().clamp_min(1e-3))
        Vq /= s
        if w is not None:
            w /= s
        Vq[:, -1] = -(z / s).median(0).values.float()

    centre(c["V0"], c["C6"], None, None)
    for l in range(1, L):
        a = evaluate(c, backward=False)
        centre(c["V"][l - 1], c["C3"], c["wt"][l - 1], torch.cat([a[f"hh{l}"], a[f"h{l}"]], 1))
    a = evaluate(c, backward=False)
    centre(c["Vp"], c["C2"], c["wtp"], torch.cat([a[f"h{l}"] for l in range(1, L + 1)], 1))
    for w, b, k in (("w3t", "b3", "y"), ("w5t", "b5", "y3")):
        z = evaluate(c, backward=False)[k] @ c[w].double()
        s = float((z - z.median(0).values).std())
        c[w] /= s
        c[b] = -(z / s).median(0).values.float()


def bernoulli_factors(c, drop, seed, swap_p=False):
    """stand-in for the kernels' counter-based factors where no GPU draws them: per site one uniform draw u, the
    factor (u >= p) / (1 - p) in fp32.  ``swap_p``: the same draws with p_layer and p_post exchanged."""
    gen = torch.Generator().manual_seed(seed)
    pl, pp = (drop[1], drop[0]) if swap_p else drop
    out = {}
    for name, p in [(f"h{l}", pl) for l in range(1, c["L"] + 1)] + [("post", pp)]:
        u = torch.rand(c["R"], H, generator=gen)
        out[name] = (u >= p).float() * torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)
    return out


# ---- the cases of tests/test_gossip_trunk_kernels_gpu.py (the host test proves each one's gate reachable) -----------
def _ladder():
    return ladder_edges()


# (name, graph, Q, regime, seed, drop settings run on it besides None)
TRUNK_CASES = [
    ("one row", lambda: (1, []), 1, "o1", 11, DROPS[:1]),
    ("ladder Q29", _ladder, 29, "aligned", 12, DROPS),
    ("ladder Q29 signed weights", _ladder, 29, "o1", 10, DROPS[:1]),
    ("permuted ladder Q3", lambda: permuted(*ladder_edges(), 5), 3, "o1", 13, DROPS[:1]),
    ("hub Q5", hub_edges, 5, "o1", 14, DROPS[1:]),
    ("Q65 N40", lambda: permuted(*prefix(40, ladder_edges()[1]), 6), 65, "o1", 15, DROPS[:1]),
    ("Q64 N20", lambda: permuted(*prefix(20, ladder_edges()[1]), 7), 64, "o1", 16, DROPS[1:]),
    ("ladder Q29 x1e6", _ladder, 29, "x1e6", 17, DROPS[:1]),
    ("ladder Q29 g1exact", _ladder, 29, "g1exact", 18, DROPS[1:]),
    ("ladder Q29 deadrelu", _ladder, 29, "deadrelu", 19, DROPS[:1]),
]
# (name, L, seed, drop settings besides None): GossipTrunkDeep on the ladder with Q = 3
DEEP_CASES = [("deep L1", 1, 21, DROPS[:1]), ("deep L2", 2, 22, DROPS[1:]), ("deep L3", 3, 23, DROPS),
              ("deep L3 signed weights", 3, 25, DROPS[1:]), ("deep L9", 9, 26, DROPS[:1])]
ALIGNED = ("ladder Q29", "deep L3", "deep L9")      # aligned weights: the cases the chain errors are measured on, and the
# 9-layer one (zero-mean weights put its mag at 1e9 times its gradients: a gate without teeth)


@functools.lru_cache(maxsize=None)
def _trunk_case(name):
    _, graph, Q, regime, seed, _ = next(c for c in TRUNK_CASES if c[0] == name)
    return case(graph(), Q, 2, "o1" if name in ALIGNED else regime, seed, "aligned" if name in ALIGNED else "signed")


@functools.lru_cache(maxsize=None)
def _deep_case(name):
    _, L, seed, _ = next(c for c in DEEP_CASES if c[0] == name)
    return case(ladder_edges(), 3, L, "o1", seed, "aligned" if name in ALIGNED else "signed")


def trunk_case(name):
    """a shallow copy of the (cached) case: set ``factors`` on it, leave its tensors alone"""
    return dict(_trunk_case(name))


def deep_case(name):
    return dict(_deep_case(name))


# ---- the formula ----------------------------------------------------------------------------------------------------
MUTATIONS = ("gate_t", "wtp_swap", "sites_swap", "dg_sign", "wt_shift")     # (p_swap is a mutation of the factors)


def _mm(a, w, chunk):
    """a @ w: whole-K, or K in ``chunk``-wide pieces summed from the last piece to the first"""
    K = w.shape[0]
    if chunk is None or K <= chunk:
        return a @ w
    acc = None
    for k in range(((K - 1) // chunk) * chunk, -1, -chunk):
        part = a[:, k:k + chunk] @ w[k:k + chunk]
        acc = part if acc is None else acc + part
    return acc


def _chains(t, P):
    """sum over dim 0 of t the way a reduction kernel with P row groups takes it: rows m = j (mod P) in ONE running sum
    each, in row order, then the P sums folded in order (train_ops.hip: the bias row of linear_bwd_w with P = 16,
    colsum_partial_kernel with P = 4); fp32 stays fp32 at every step"""
    n = t.shape[0]
    pad = (-n) % P
    if pad:
        t = torch.cat([t, torch.zeros((pad,) + tuple(t.shape[1:]), dtype=t.dtype)])
    acc = torch.zeros((P,) + tuple(t.shape[1:]), dtype=t.dtype)
    for m in range(0, n + pad, P):
        acc = acc + t[m:m + P]
    out = acc[0]
    for j in range(1, P):
        out = out + acc[j]
    return out


def _rowsum(fn, rows, chunk):
    """sum over the rows of fn(r0, r1) (a function of a row range): whole, or in pieces of 8 chunk rows, last first"""
    if chunk is None or rows <= 8 * chunk:
        return fn(0, rows)
    acc = None
    for r0 in range(((rows - 1) // (8 * chunk)) * 8 * chunk, -1, -8 * chunk):
        part = fn(r0, min(rows, r0 + 8 * chunk))
        acc = part if acc is None else acc + part
    return acc


def evaluate(c, dtype=torch.float64, pins=None, chunk=None, absolute=False, backward=True, mutate=None, chains=None):
    """``chains`` = P: a third summation order for the column sums (db3, db5, db7) and the node sum of dg_l, see _chains"""
    assert mutate is None or mutate in MUTATIONS
    conv = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))    # noqa: E731
    G, N, Q, L, R = c["G"], c["N"], c["Q"], c["L"], c["R"]
    src, dst = (G.src, G.dst) if chunk is None else (G.src.flip(0), G.dst.flip(0))
    lo = dst < src
    C6, C3, C2, x = conv(c["C6"]), conv(c["C3"]), conv(c["C2"]), conv(c["x"]).reshape(-1)
    V0, Vp, wtp, w3t, b3, w5t, b5, w7, b7, dpred = (conv(c[k]) for k in ("V0", "Vp", "wtp", "w3t", "b3", "w5t", "b5", "w7",
                                                                       "b7", "dpred"))
    g, wt, V = [conv(t) for t in c["g"]], [conv(t) for t in c["wt"]], [conv(t) for t in c["V"]]
    one = torch.ones((), dtype=dtype)
    fac = (lambda k: one) if c["factors"] is None else (lambda k: c["factors"][k].to(dtype))    # noqa: E731
    slope = lambda m: m + 0.1 * (1 - m)                                               # noqa: E731

    def act(z, name, leaky=False):
        if pins is not None:
            m = (pins[name] > 0).to(dtype).reshape(z.shape)
            return z * (slope(m) if leaky else m)
        if absolute:
            return z
        return torch.where(z > 0, z, 0.1 * z) if leaky else torch.relu(z)

    def dact(out, name, leaky=False):
        """act'(c) from the activation output: the pinned one, else this evaluation's own"""
        m = ((pins[name] if pins is not None else out) > 0).to(dtype).reshape(out.shape)
        if pins is None and absolute:
            m = torch.ones_like(out)
        return slope(m) if leaky else m

    def affine(C, Vq):
        return torch.einsum("nqk,qkc->nqc", C.view(N, Q, -1), Vq).reshape(R, H)

    def affine_bwd(C, dz):
        k = C.shape[1]
        return _rowsum(lambda a, b: torch.einsum("nqk,nqc->qkc", C.view(N, Q, k)[a:b], dz.view(N, Q, H)[a:b]), N, chunk)

    def gather(h, w_lo, w_hi):
        """out[i, q] = sum_{j ~ i} (j < i ? w_lo[q] : w_hi[q]) h[j, q]"""
        w = torch.where(lo[:, None], w_lo[None, :], w_hi[None, :])                      # [E, Q]
        return torch.zeros(N, Q, H, dtype=dtype).index_add_(0, src, w[:, :, None] * h.view(N, Q, H)[dst]).reshape(R, H)

    ones_q = torch.ones(Q, dtype=dtype)
    # ---- forward ----
    h, hh = [None] * (L + 1), [None] * L
    h[1] = fac("h1") * act(affine(C6, V0), "h1")
    for l in range(1, L):
        hh[l] = gather(h[l], g[l - 1], 1 - g[l - 1])
        h[l + 1] = fac(f"h{l + 1}") * act(_mm(torch.cat([hh[l], h[l]], 1), wt[l - 1], chunk) + affine(C3, V[l - 1]), f"h{l + 1}")
    hcat = torch.cat(h[1:], 1)
    y = fac("post") * act(_mm(hcat, wtp, chunk) + affine(C2, Vp), "y", leaky=True)
    y3 = act(_mm(y, w3t, chunk) + b3, "y3")
    y5 = act(_mm(y3, w5t, chunk) + b5, "y5")
    pred = x + b7 + _mm(y5, w7[:, None], chunk)[:, 0]
    out = {f"h{l}": h[l] for l in range(1, L + 1)}
    out.update({f"hh{l}": hh[l] for l in range(1, L)})
    out.update(y=y, y3=y3, y5=y5, pred=pred)
    if not backward:
        return out
    # ---- backward ----
    tmm = lambda a, dz: _rowsum(lambda r0, r1: a[r0:r1].t() @ dz[r0:r1], R, chunk)    # noqa: E731
    colsum = (lambda dz: _chains(dz, chains)) if chains else (                          # noqa: E731
        lambda dz: _rowsum(lambda r0, r1: dz[r0:r1].sum(0), R, chunk))
    f_post, f_h2 = fac("post"), (fac("h2") if L >= 2 else None)
    if mutate == "sites_swap":
        assert L >= 2
        f_post, f_h2 = fac("h2"), fac("post")
    out["dw7"], out["db7"] = tmm(dpred[:, None], y5)[0], colsum(dpred[:, None])
    dz5 = dpred[:, None] * w7[None, :] * dact(y5, "y5")
    out["dw5t"], out["db5"] = tmm(y3, dz5), colsum(dz5)
    dz3 = _mm(dz5, w5t.t(), chunk) * dact(y3, "y3")
    out["dw3t"], out["db3"] = tmm(y, dz3), colsum(dz3)
    dzp = _mm(dz3, w3t.t(), chunk) * f_post * dact(y, "y", leaky=True)
    out["dwtp"], out["dVp"] = tmm(hcat, dzp), affine_bwd(C2, dzp)
    blk = list(range(L))
    if mutate == "wtp_swap":
        assert L >= 2
        blk[0], blk[1] = 1, 0
    dh = [None] + [_mm(dzp, wtp[H * blk[l]:H * (blk[l] + 1)].t(), chunk) for l in range(L)]
    for l in range(L - 1, 0, -1):                                                       # layer l: h_l -> h_{l+1}
        fl = f_h2 if l == 1 else fac(f"h{l + 1}")
        dz = dh[l + 1] * fl * dact(h[l + 1], f"h{l + 1}")
        out[f"dV{l}"], out[f"dwt{l}"] = affine_bwd(C3, dz), tmm(torch.cat([hh[l], h[l]], 1), dz)
        w = wt[l - 2] if (mutate == "wt_shift" and l >= 2) else wt[l - 1]
        dhh = _mm(dz, w[:H].t(), chunk)
        gl = g[l - 1]
        # transpose of the gated sum: node j receives (i > j ? g : 1 - g) dhh[i] from each neighbour i
        dh[l] = dh[l] + _mm(dz, w[H:].t(), chunk) + (gather(dhh, gl, 1 - gl) if mutate == "gate_t" else gather(dhh, 1 - gl, gl))
        # d hh / d g = sum_{j<i} h_j - sum_{j>i} h_j
        sig = gather(h[l], ones_q, ones_q if (absolute or mutate == "dg_sign") else -ones_q)
        rd = (dhh * sig).sum(1).view(N, Q)
        out[f"dg{l}"] = _chains(rd, chains) if chains else _rowsum(lambda a, b: rd[a:b].sum(0), N, chunk)
    dz0 = dh[1] * fac("h1") * dact(h[1], "h1")
    out["dV0"] = affine_bwd(C6, dz0)
    return out


def mag(c, pins=None, backward=True):
    return evaluate(c, torch.float64, pins, None, absolute=True, backward=backward)


ACTIVATIONS = lambda L: [f"h{l}" for l in range(1, L + 1)] + [f"hh{l}" for l in range(1, L)] + ["y", "y3", "y5", "pred"]   # noqa: E731
GRADIENTS = lambda L: ["dV0"] + [f"{k}{l}" for l in range(1, L) for k in ("dg", "dwt", "dV")] + [                             # noqa: E731
    "dwtp", "dVp", "dw3t", "db3", "dw5t", "db5", "dw7", "db7"]


def pins_of(acts):
    """the activations relu' / leaky' are read from, out of a dict of activations (any float dtype, any device)"""
    return {k: v.detach().cpu() for k, v in acts.items() if k == "y" or k == "y3" or k == "y5" or (k[0] == "h" and k[1] != "h")}


def scaled_error(got, ref, m):
    """(E = max |got - ref| / mag over the elements, flat index of the worst one); an exact element counts 0 whatever
    mag, a wrong one at mag 0 counts inf"""
    err = (got.double().reshape(ref.shape) - ref).abs()
    e = torch.where(err == 0, torch.zeros_like(err), err / m)
    e = torch.nan_to_num(e, nan=float("inf"))
    i = int(e.flatten().argmax()) if e.numel() else 0
    return (float(e.flatten()[i]) if e.numel() else 0.0), i
