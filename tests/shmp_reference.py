"""Host reference of the SHMP training trunk (autograd.ShmpTrunk's docstring; header of csrc/shmp_small.hip), written
from the documented contract alone: numpy + torch, ``index_add_`` over explicit index lists, backward by torch autograd,
no call into ``desco_amd.ops`` or ``desco_amd.autograd``.  Used by tests/test_shmp_trunk_kernels_gpu.py (the kernels and
the autograd nodes against it) and by tests/test_shmp_reference_host.py (the reference against a dense-matrix formula,
and the gate against a second fp32 summation order).

    X_0 = x0;   A_l = [agg_0(X_l) .. agg_{su-1}(X_l) | X_l]   (agg_s: sum over the sources of virtual row i slots + s)
    X_{l+1} = factor_l * relu(A_l Wt_l + b_l)                  (per row group (r0, r1, su): its own Wt, bias)
    pooled[:, 64 l : 64 (l+1)] = segment sum of X_l over seg_ptr  (+ block l of leaky_0.1(canon aw + ab), where
                                 canon[b] = [X_0[Nc + b] | .. | X_L[Nc + b]], Nc = seg_ptr[B]: the anchor)

A *case* is a dict: x0 [N, 64], vrowptr, vcol (int64 tensors), slots, groups [(r0, r1, su)], Wt / bias (one stacked
tensor per group), seg_ptr (int64 tensor [B + 1]), B, anchor (aw [P, P] K-major, ab [P]) or None, factors (per layer
[N, 64]) or None, dpooled [B, 64 (L + 1)].  ``evaluate`` returns every X_l, pooled and -- from dpooled -- the gradients
of x0 and of every weight and bias, in the dtype asked for: float64 is the reference, float32 the *fp32 evaluation* the
kernels are held to.  ``pins`` (per layer a 0/1 tensor [N, 64], X_{l+1} > 0 of activations the caller supplies) replaces
relu by multiplication with that mask; ``anchor_pin`` does the same for the sign of the anchor's pre-activation.
``absolute=True`` evaluates the same function on |x0|, |Wt|, |bias|, |anchor|, |dpooled| with factors and pins kept and
the remaining relu / leaky replaced by identity: on non-negative inputs that is the sum of |terms| of every output and
gradient, the scale their rounding errors live on (``mag``)."""
import numpy as np
import torch

H = 64


# ---- graphs and their virtual-row CSR -------------------------------------------------------------------------------
def query_csr(graphs):
    """[(n, edges)] -> (vrowptr [2 N + 1], vcol, seg_ptr [B + 1]) int64 tensors of the union of the graphs: virtual row
    2 i + s holds the neighbours j of row i over triangle edges (s = 0: i and j share a neighbour) or over the others
    (s = 1), ascending."""
    ents, off, seg = [], 0, [0]
    for n, edges in graphs:
        nb = [set() for _ in range(n)]
        for a, b in edges:
            if a != b:
                nb[a].add(b)
                nb[b].add(a)
        for i in range(n):
            for j in nb[i]:
                ents.append((2 * (off + i) + (0 if nb[i] & nb[j] else 1), off + j))
        off += n
        seg.append(off)
    ents.sort()
    cnt = np.bincount(np.array([v for v, _ in ents], dtype=np.int64), minlength=2 * off) if ents else np.zeros(2 * off, np.int64)
    vrowptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    vcol = np.array([c for _, c in ents], dtype=np.int64)
    return torch.from_numpy(vrowptr), torch.from_numpy(vcol), torch.tensor(seg, dtype=torch.int64)


def clique(k):
    return k, [(a, b) for a in range(k) for b in range(a + 1, k)]


def path(k):
    return k, [(a, a + 1) for a in range(k - 1)]


def ring(k, chords=()):
    return k, [(a, (a + 1) % k) for a in range(k)] + list(chords)


def wheel(n):
    """hub 0 joined to a rim cycle 1..n-1: every edge lies in a triangle (the hub row has n - 1 slot-0 sources)"""
    return n, [(0, v) for v in range(1, n)] + [(v, v + 1) for v in range(1, n - 1)] + [(n - 1, 1)]


def star(n):
    """centre n // 2 joined to every other id: no triangle (the centre row has n - 1 slot-1 sources)"""
    c = n // 2
    return n, [(c, v) for v in range(n) if v != c]


def random_graph(n, seed):
    rng = np.random.default_rng(seed)
    e = [(int(rng.integers(v)), v) for v in range(1, n)]
    e += [(int(rng.integers(n)), int(rng.integers(n))) for _ in range(2 * n)]
    return n, e


SHAPES = [clique(1), clique(2), path(3), clique(3), path(4), ring(4), clique(4), path(5), ring(5, [(0, 2)]), path(6),
          ring(6, [(0, 3), (1, 3)]), path(7), clique(7), path(8), ring(8, [(0, 4), (1, 5), (0, 2)]), clique(8)]


def mixed_graphs(n, seed, lo=1, hi=8):
    """graphs of lo..hi rows from SHAPES (paths, rings, cliques up to K8) with ``n`` rows in all"""
    rng = np.random.default_rng(seed)
    pool = [g for g in SHAPES if lo <= g[0] <= hi]
    out, left = [], n
    while left > 0:
        fit = [g for g in pool if g[0] <= left]
        g = fit[int(rng.integers(len(fit)))] if fit else path(left)
        out.append(g)
        left -= g[0]
    return out


# ---- the cases of tests/test_shmp_trunk_kernels_gpu.py (the host test proves each one's gate reachable) ----------------
# (name, graphs, L, regime, dpooled strided).  One-workgroup kernels: at most 144 rows, graphs of any size.
SMALL_CASES = [(f"n{n}", mixed_graphs(n, n), L, "o1", i % 2 == 1)
               for i, (n, L) in enumerate([(1, 2), (2, 2), (21, 3), (22, 8), (63, 1), (64, 2), (65, 3), (128, 8), (129, 1),
                                           (143, 2), (144, 3)])] + [
    ("one graph of 144 rows", [random_graph(144, 7)], 3, "o1", False),
    ("144 graphs of one row", [clique(1)] * 144, 2, "o1", True),
    ("wheel on 144 rows", [wheel(144)], 2, "o1", False),
    ("star on 144 rows", [star(144)], 1, "o1", True),
    ("n135 L12", mixed_graphs(135, 12, 3, 5), 12, "o1", False),
    ("dead relu", mixed_graphs(100, 31), 3, "deadrelu", True),
    ("rows 2^+-16", mixed_graphs(100, 32), 2, "range", False),
]
# per-graph kernels: graphs of at most 8 rows, any number of rows
GRAPH_CASES = [
    ("every shape 1..8", list(SHAPES), 2, "o1", False),
    ("n127", mixed_graphs(127, 127), 1, "o1", True),
    ("n128", mixed_graphs(128, 128), 3, "o1", False),
    ("n129", mixed_graphs(129, 129), 8, "o1", True),
    ("3000 rows", mixed_graphs(3000, 5, 4, 8), 2, "o1", False),
    ("2500 graphs", mixed_graphs(3700, 6, 1, 2), 1, "o1", True),
    ("dead relu", mixed_graphs(100, 31), 3, "deadrelu", True),
    ("rows 2^+-16", mixed_graphs(100, 32), 2, "range", False),
]
DROP_CASES = [("dropout 0.01", list(SHAPES) * 3, 3, 0.01, 5), ("dropout 0.3", list(SHAPES) * 3, 2, 0.3, 40)]   # .., p, site
DEAD_COLS, ZERO_COLS = slice(16, 32), slice(32, 36)


def operands(N, B, L, regime, seed, groups=((0, None, 2),), anchor=False):
    """fp32 operands of one case: x0 [N, 64], per group Wt [L, (su + 1) 64, 64] and bias [L, 64], dpooled [B, 64 (L + 1)],
    (aw, ab) if anchor.  ``deadrelu``: columns DEAD_COLS of every layer far below zero, columns ZERO_COLS with zero
    weights and bias (pre-activation exactly 0 in any arithmetic).  ``range``: the rows of x0 scaled by 2^-16 .. 2^16."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                       # noqa: E731
    x0 = r(N, H)
    Wt = [r(L, (su + 1) * H, H) / 10 for _, _, su in groups]
    bias = [r(L, H) / 4 for _ in groups]
    P = H * (L + 1)
    dpooled = r(B, P)
    if regime == "deadrelu":
        for w, b in zip(Wt, bias):
            b[:, DEAD_COLS] = -1e3
            w[:, :, ZERO_COLS] = 0
            b[:, ZERO_COLS] = 0
    elif regime == "range":
        x0 = x0 * 2.0 ** torch.randint(-16, 17, (N, 1), generator=g).float()
    out = dict(x0=x0, Wt=Wt, bias=bias, dpooled=dpooled, anchor=None)
    if anchor:
        out["anchor"] = (r(P, P) / np.sqrt(P), r(P) / 4)
    return out


def query_case(graphs, L, regime, seed, factors=None):
    """the single-group case (two relation slots, no anchor) of a list of graphs"""
    vrowptr, vcol, seg_ptr = query_csr(graphs)
    N, B = int(seg_ptr[-1]), len(graphs)
    c = operands(N, B, L, regime, seed)
    c.update(vrowptr=vrowptr, vcol=vcol, slots=2, groups=[(0, N, 2)], seg_ptr=seg_ptr, B=B, factors=factors)
    return c


def neighborhood_case(vrowptr, vcol, count_ptr, num_rows, L, seed, factors=None):
    """the two-group case of a neighborhood batch: num_count count rows (4 relation slots) followed by one canonical row
    per neighborhood (the first 2 of its 4 slots), pooling over the count rows, the anchor on the canonical rows"""
    as64 = lambda a: torch.as_tensor(np.asarray(a).astype(np.int64))                  # noqa: E731
    count_ptr = as64(count_ptr)
    B, Nc = len(count_ptr) - 1, int(count_ptr[-1])
    assert num_rows == Nc + B
    groups = [(0, Nc, 4), (Nc, num_rows, 2)]
    c = operands(num_rows, B, L, "o1", seed, groups, anchor=True)
    c.update(vrowptr=as64(vrowptr), vcol=as64(vcol), slots=4, groups=groups, seg_ptr=count_ptr, B=B, factors=factors)
    return c


def bernoulli_factors(N, L, p, seed):
    """stand-in for the kernels' counter-based factors where no GPU draws them: 0 or 1 / (1 - p) (fp32), per layer"""
    g = torch.Generator().manual_seed(seed)
    s = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)
    return [(torch.rand(N, H, generator=g) >= p).float() * s for _ in range(L)]


# ---- the formula ----------------------------------------------------------------------------------------------------
def _mm(a, w, chunk):
    """a @ w: whole-K, or K in ``chunk``-wide pieces summed from the last piece to the first"""
    if chunk is None:
        return a @ w
    acc = None
    for k in range(w.shape[0] - chunk, -1, -chunk):
        part = a[:, k:k + chunk] @ w[k:k + chunk]
        acc = part if acc is None else acc + part
    return acc


def trunk(x0, vrowptr, vcol, slots, groups, Wt, bias, seg_ptr, B, anchor=None, factors=None, pins=None, anchor_pin=None,
          chunk=None, relu=True):
    """([X_0 .. X_L], pooled [B, 64 (L + 1)], the anchor block [B, 64 (L + 1)] or None) in the dtype of x0;
    differentiable.  relu=False: identity activations."""
    N, L = x0.shape[0], Wt[0].shape[0]
    vrow = torch.repeat_interleave(torch.arange(N * slots), vrowptr[1:] - vrowptr[:-1])
    X = [x0]
    for l in range(L):
        agg = torch.zeros(N * slots, H, dtype=x0.dtype).index_add_(0, vrow, X[-1][vcol]).view(N, slots * H)
        z = torch.cat([_mm(torch.cat([agg[r0:r1, :su * H], X[-1][r0:r1]], 1), Wt[g][l], chunk) + bias[g][l]
                       for g, (r0, r1, su) in enumerate(groups)])
        assert z.shape[0] == N, "the row groups tile the rows in order"
        x = z * pins[l] if pins is not None else (torch.relu(z) if relu else z)
        X.append(x if factors is None else x * factors[l])
    Nc = int(seg_ptr[B])
    seg = torch.repeat_interleave(torch.arange(B), seg_ptr[1:] - seg_ptr[:-1])
    pooled = torch.cat([torch.zeros(B, H, dtype=x0.dtype).index_add_(0, seg, x[:Nc]) for x in X], 1)
    a = None
    if anchor is not None:
        a = _mm(torch.cat([x[Nc:Nc + B] for x in X], 1), anchor[0], chunk) + anchor[1]
        if anchor_pin is not None:
            a = a * (anchor_pin + 0.1 * (1 - anchor_pin))
        elif relu:
            a = torch.where(a > 0, a, 0.1 * a)
        pooled = pooled + a
    return X, pooled, a


def evaluate(case, dtype=torch.float64, chunk=None, pins=None, anchor_pin=None, absolute=False, backward=True):
    """dict: xall [L, N, 64], pooled, (anchor) anch, and (backward) dx0, dwt{g}, dbias{g}, daw, dab from case["dpooled"]"""
    conv = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))    # noqa: E731
    leaf = lambda t: conv(t).clone().requires_grad_(backward)                         # noqa: E731
    x0 = leaf(case["x0"])
    Wt, bias = [leaf(w) for w in case["Wt"]], [leaf(b) for b in case["bias"]]
    anchor = None if case.get("anchor") is None else tuple(leaf(t) for t in case["anchor"])
    keep = lambda ts: None if ts is None else [t.to(dtype) for t in ts]               # noqa: E731
    X, pooled, anch = trunk(x0, case["vrowptr"], case["vcol"], case["slots"], case["groups"], Wt, bias, case["seg_ptr"],
                      case["B"], anchor, keep(case.get("factors")), keep(pins),
                      None if anchor_pin is None else anchor_pin.to(dtype), chunk, relu=not absolute)
    out = {"xall": torch.stack(X[1:]).detach(), "pooled": pooled.detach()}
    if anch is not None:
        out["anch"] = anch.detach()
    if backward:
        pooled.backward(conv(case["dpooled"]))
        out["dx0"] = x0.grad
        for g in range(len(Wt)):
            out[f"dwt{g}"], out[f"dbias{g}"] = Wt[g].grad, bias[g].grad
        if anchor is not None:
            out["daw"], out["dab"] = anchor[0].grad, anchor[1].grad
    return out


def mag(case, pins=None, anchor_pin=None, backward=True):
    return evaluate(case, torch.float64, None, pins, anchor_pin, absolute=True, backward=backward)


def pins_of(xall):
    """the relu masks X_{l+1} > 0 of activations [L, N, 64] (any float dtype)"""
    return [(x > 0).double() for x in xall]


def scaled_error(got, ref, m):
    """(E = max |got - ref| / mag over the elements, flat index of the worst one); an exact element counts 0 whatever
    mag, a wrong one at mag 0 counts inf"""
    err = (got.double().reshape(ref.shape) - ref).abs()
    e = torch.where(err == 0, torch.zeros_like(err), err / m)
    e = torch.nan_to_num(e, nan=float("inf"))
    i = int(e.flatten().argmax()) if e.numel() else 0
    return (float(e.flatten()[i]) if e.numel() else 0.0), i
