"""The SHMP training trunks -- the five kernels of csrc/shmp_small.hip through ops.shmp_trunk_small_* /
ops.shmp_trunk_graphs_*, and the autograd nodes ShmpTrunkSmall / ShmpTrunk -- per element against the fp64 host
reference tests/shmp_reference.py.

Gate (the gossip kernels' precedent, tests/test_gossip_kernels_gpu.py; no number of its own): per tensor
E_kernel = max |got - ref| / mag over ALL elements, mag = the reference evaluated on absolute values (the sum of |terms|
of the element).  E_kernel <= 4 E_f32, where E_f32 is the same figure of the reference evaluated in float32 on the host
on the same case, and E_kernel <= 1e-4 (the ceiling of tests/test_train_kernels_gpu.py).  An element with mag == 0 must
be exactly 0.  tests/test_shmp_reference_host.py proves the gate reachable: a second fp32 summation order stays within
the factor 4 on every case below.

The forward is compared with the unpinned reference.  The backward is fed the ``xall`` its own forward produced (after
that forward has passed) and the reference backward pins its relu masks to that same ``xall``, so that a pre-activation
within rounding of zero does not become a discontinuous gradient difference.  Every test prints E_kernel, E_f32 and
their ratio as ``[parity]`` lines; the worst ratio per tensor is printed once more when the module ends."""
import collections

import pytest
import torch

pytestmark = pytest.mark.gpu

import shmp_reference as R  # noqa: E402
from desco_amd import autograd as AG  # noqa: E402
from desco_amd import ops  # noqa: E402
from desco_amd.batch import QueryBatch  # noqa: E402

DEV = "cuda"
H = R.H
CEILING = 1e-4
WORST = collections.defaultdict(float)          # tensor -> worst E_kernel / E_f32 seen


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    for k in sorted(WORST):
        print(f"[parity] trunk worst E_kernel / E_f32 over the module, {k}: {WORST[k]:.2f} (gate 4)")


def _gate(name, got, ref, mag, f32, keys, family):
    """E_kernel <= 4 E_f32 and <= CEILING for every tensor of ``keys``; zero where mag is zero"""
    bad = []
    for k in keys:
        g = got[k].detach().cpu().double().reshape(ref[k].shape)
        ek, i = R.scaled_error(g, ref[k], mag[k])
        ef, _ = R.scaled_error(f32[k], ref[k], mag[k])
        ratio = ek / ef if ef > 0 else (0.0 if ek == 0 else float("inf"))
        WORST[f"{family} {k.rstrip('0123456789')}"] = max(WORST[f"{family} {k.rstrip('0123456789')}"], ratio)
        print(f"[parity] {name} {k}: E_kernel {ek:.3e}, E_f32 {ef:.3e}, ratio {ratio:.2f} (gate 4, ceiling {CEILING:.0e})")
        exact = bool((g[mag[k] == 0] == 0).all())
        if not (ek <= 4 * ef and ek <= CEILING and exact):
            bad.append(f"{name} {k}: E_kernel {ek:.3e} E_f32 {ef:.3e} ratio {ratio:.2f}; element {i}: got "
                       f"{float(g.flatten()[i])!r}, ref {float(ref[k].flatten()[i])!r}, mag {float(mag[k].flatten()[i])!r}"
                       f"{'' if exact else '; nonzero where mag == 0'}")
    assert not bad, "\n".join(bad)


def _bit_identical(name, a, b):
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), f"{name}: two launches on the same inputs differ"


def _dpooled(case, strided):
    """case["dpooled"] on the device: contiguous, or a column-strided view (ldp = 64 (L + 1) + 12, 32 bytes in)"""
    dp = case["dpooled"]
    if not strided:
        return dp.to(DEV)
    buf = torch.full((dp.shape[0], dp.shape[1] + 12), float("nan"))
    buf[:, 8:8 + dp.shape[1]] = dp
    view = buf.to(DEV)[:, 8:8 + dp.shape[1]]
    assert view.stride(0) > dp.shape[1] and view.data_ptr() % 16 == 0
    return view


def _batch(graphs, case):
    """the product's own batch of the case's graphs: its index is the reference's"""
    qb = QueryBatch(graphs, DEV)
    assert torch.equal(qb.vrowptr.cpu().long(), case["vrowptr"]) and torch.equal(qb.vcol.cpu().long(), case["vcol"])
    assert torch.equal(qb.graph_ptr.cpu().long(), case["seg_ptr"])
    return qb


def _run_kernels(kind, name, graphs, L, regime, strided, seed, drop=None):
    """forward, then backward, of the one-workgroup (``small``) or per-graph (``graphs``) entry points on one case"""
    case = R.query_case(graphs, L, regime, seed)
    qb = _batch(graphs, case)
    n, B = qb.num_rows, qb.num_graphs
    if kind == "graphs":
        assert int((case["seg_ptr"][1:] - case["seg_ptr"][:-1]).max()) <= ops.shmp_trunk_graphs_max_rows()
    else:
        assert n <= ops.shmp_trunk_small_max_rows()
    x0, wt, bias = case["x0"].to(DEV), case["Wt"][0].to(DEV), case["bias"][0].to(DEV)
    mask_scale, kw = 1.0, {}
    if drop is not None:
        key, site, p = drop
        kw = dict(drop=ops.DropSite(key, site, p))
        mask_scale = kw["drop"].scale
        case["factors"] = [ops.dropout_mask(ops.DropSite(key, site + 2 * l, p), n, H).cpu() for l in range(L)]
        assert all((f == 0).any() and (f != 0).any() for f in case["factors"])
    fwd = ops.shmp_trunk_small_fwd if kind == "small" else ops.shmp_trunk_graphs_fwd
    xall, pooled = fwd(x0, qb.vrowptr, qb.vcol, wt, bias, qb.graph_ptr, B, **kw)
    _bit_identical(f"{kind} fwd {name}", (xall, pooled), fwd(x0, qb.vrowptr, qb.vcol, wt, bias, qb.graph_ptr, B, **kw))
    ref, m = R.evaluate(case, backward=False), R.mag(case, backward=False)
    f32 = R.evaluate(case, torch.float32, backward=False)
    tag = f"{kind} kernels, {name} (n {n}, B {B}, L {L})"
    _gate(tag, dict(xall=xall, pooled=pooled), ref, m, f32, ("xall", "pooled"), f"{kind} kernels")
    if drop is not None:                       # the masks matter
        plain = fwd(x0, qb.vrowptr, qb.vcol, wt, bias, qb.graph_ptr, B)[1]
        assert float(((pooled - plain).abs() / (1 + plain.abs())).max()) > 1e-3
    # backward on the kernel's own activations; the reference pinned to them
    dp = _dpooled(case, strided)
    ti = qb.train_index()
    if kind == "small":
        wt_t = wt.transpose(1, 2).contiguous()
        run = lambda: ops.shmp_trunk_small_bwd(x0, xall, qb.vrowptr, qb.vcol, ti["t_rowptr"], ti["t_col_s1"],      # noqa: E731
                                               ti["seg_id"], wt_t, dp)
    else:
        run = lambda: ops.shmp_trunk_graphs_bwd(x0, xall, qb.vrowptr, qb.vcol, ti["t_rowptr"], ti["t_col_s1"],     # noqa: E731
                                                qb.graph_ptr, B, wt, dp, mask_scale)
    dwt, dbias, dx0 = run()
    _bit_identical(f"{kind} bwd {name}", (dwt, dbias, dx0), run())
    pins = R.pins_of(xall.cpu())
    ref, m, f32 = R.evaluate(case, pins=pins), R.mag(case, pins), R.evaluate(case, torch.float32, pins=pins)
    _gate(tag + (", strided dpooled" if strided else ""), dict(dwt0=dwt, dbias0=dbias, dx0=dx0), ref, m, f32,
          ("dwt0", "dbias0", "dx0"), f"{kind} kernels")
    if regime == "deadrelu":
        for cols in (R.DEAD_COLS, R.ZERO_COLS):
            assert not xall[..., cols].any() and not dbias[:, cols].any() and not dwt[..., cols].any()
    return case, xall


_SMALL = [(f"{n}", g, L, r, s, 100 + i) for i, (n, g, L, r, s) in enumerate(R.SMALL_CASES)] + \
         [(f"{n} (per-graph case)", g, L, r, s, 200 + i) for i, (n, g, L, r, s) in enumerate(R.GRAPH_CASES)
          if sum(k for k, _ in g) <= 144]
_GRAPHS = [(f"{n}", g, L, r, s, 200 + i) for i, (n, g, L, r, s) in enumerate(R.GRAPH_CASES)] + \
          [(f"{n} (one-workgroup case)", g, L, r, s, 100 + i) for i, (n, g, L, r, s) in enumerate(R.SMALL_CASES)
           if max(k for k, _ in g) <= 8]


@pytest.mark.parametrize("name,graphs,L,regime,strided,seed", _SMALL, ids=[c[0] for c in _SMALL])
def test_one_workgroup_kernels_match_the_reference(name, graphs, L, regime, strided, seed):
    """shmp_small_fwd_kernel / shmp_small_bwd_kernel: row counts on both sides of the forward's 64-row and the
    backward's 21-row tiling up to the 144-row limit, one large graph, graphs without edges, hub rows in either slot,
    L from 1 to 12, dead columns, rows at 2^+-16, contiguous and strided dpooled; each launched twice."""
    assert {c[2] for c in _SMALL} >= {1, 2, 3, 8, 12}
    _run_kernels("small", name, graphs, L, regime, strided, seed)


@pytest.mark.parametrize("name,graphs,L,regime,strided,seed", _GRAPHS, ids=[c[0] for c in _GRAPHS])
def test_per_graph_kernels_match_the_reference(name, graphs, L, regime, strided, seed):
    """shmp_graphs_fwd_kernel / shmp_graphs_bwd_kernel / shmp_graphs_bwd_w_kernel: graphs of 1..8 rows (K8, paths), row
    counts around the weight-gradient kernel's 128-row chunk, thousands of rows (many chunks), thousands of segments."""
    _run_kernels("graphs", name, graphs, L, regime, strided, seed)


@pytest.mark.parametrize("name,graphs,L,p,site", R.DROP_CASES, ids=[c[0] for c in R.DROP_CASES])
def test_per_graph_kernels_with_dropout_match_the_reference(name, graphs, L, p, site):
    """drop=DropSite(key, site, p) with a nonzero base site: the reference is fed ops.dropout_mask of site + 2 l, the
    backward runs with mask_scale = 1 / (1 - p); the masks change the result."""
    ops.manual_seed(4242, step=7)
    key = ops.rng_next(DEV)
    assert site > 0
    case, xall = _run_kernels("graphs", name, graphs, L, "o1", False, 300 + site, drop=(key, site, p))
    kept = torch.stack(case["factors"]) != 0
    assert not xall.cpu()[~kept].any()
    assert abs(float(kept.float().mean()) - (1 - p)) < 0.02


# ---- the autograd nodes -----------------------------------------------------------------------------------------------
def _node_grads(case, pooled, leaves):
    (pooled * case["dpooled"].to(DEV)).sum().backward()
    return [t.grad for t in leaves]


def _gate_node(tag, family, case, pooled_t, grads, xall, anch=None):
    """pooled against the unpinned reference, the gradients against the reference pinned to the node's activations"""
    ref, m = R.evaluate(case, backward=False), R.mag(case, backward=False)
    f32 = R.evaluate(case, torch.float32, backward=False)
    _gate(tag, dict(pooled=pooled_t), ref, m, f32, ("pooled",), family)
    pins = R.pins_of(xall.cpu())
    apin = None if anch is None else (anch.cpu() > 0).double()
    ref, m = R.evaluate(case, pins=pins, anchor_pin=apin), R.mag(case, pins, apin)
    f32 = R.evaluate(case, torch.float32, pins=pins, anchor_pin=apin)
    _gate(tag, grads, ref, m, f32, tuple(grads), family)


@pytest.mark.parametrize("per_graph", [True, False])
@pytest.mark.parametrize("p", [None, 0.2])
@pytest.mark.parametrize("layers", [1, 8])
def test_small_node_matches_the_reference(per_graph, p, layers):
    """autograd.ShmpTrunkSmall in both forms (``_small_per_graph``), with and without dropout (the per-graph form
    only: the node refuses dropout in the one-workgroup form), on the standard queries and on graphs of 1..8 rows."""
    from helpers import standard_queries
    for name, graphs in (("standard queries", standard_queries()[1]), ("every shape 1..8", list(R.SHAPES))):
        case = R.query_case(graphs, layers, "o1", 500 + layers)
        qb = _batch(graphs, case)
        assert AG.ShmpTrunkSmall.per_graph(qb)
        qb.__dict__["_small_per_graph"] = per_graph
        a, w, b = (t.clone().to(DEV).requires_grad_() for t in (case["x0"], case["Wt"][0], case["bias"][0]))
        drop = None
        if p is not None:
            ops.manual_seed(99, step=3)
            drop = (ops.rng_next(DEV), p)
            if not per_graph:
                with pytest.raises(AssertionError):
                    AG.ShmpTrunkSmall.apply(a, qb, drop, w, b)
                continue
            case["factors"] = [ops.dropout_mask(ops.DropSite(drop[0], 2 * l, p), qb.num_rows, H).cpu()
                               for l in range(layers)]
        pooled = AG.ShmpTrunkSmall.apply(a, qb, drop, w, b)
        xall = pooled.grad_fn.saved_tensors[1]
        assert tuple(xall.shape) == (layers, qb.num_rows, H)
        dx0, dwt, dbias = _node_grads(case, pooled, (a, w, b))
        _gate_node(f"ShmpTrunkSmall {'per-graph' if per_graph else 'one-workgroup'}, {name}, L {layers}, dropout {p}",
                   "small node", case, pooled.detach(), dict(dx0=dx0, dwt0=dwt, dbias0=dbias), xall)


def _node_names(t):
    seen, stack = set(), [t.grad_fn]
    while stack:
        f = stack.pop()
        if f is not None and f not in seen:
            seen.add(f)
            stack += [n for n, _ in f.next_functions]
    return {type(f).__name__ for f in seen}


def test_a_dropout_batch_with_a_9_row_graph_takes_the_general_node():
    """gnn_model.shmp_forward_train: the per-graph kernels (the only small ones that carry dropout) clamp a graph of
    more than 8 rows, so a dropout step on such a batch must run autograd.ShmpTrunk; without dropout it keeps the
    one-workgroup form of ShmpTrunkSmall, and a batch of small graphs keeps ShmpTrunkSmall with dropout."""
    from helpers import neigh_args
    from desco_amd.lightning_model import NeighborhoodCountingModel
    nine = [R.path(9), R.clique(3)]
    assert not AG.ShmpTrunkSmall.per_graph(QueryBatch(nine, DEV))
    for p, graphs, want in ((0.2, nine, "ShmpTrunkBackward"), (0.0, nine, "ShmpTrunkSmallBackward"),
                            (0.2, [R.path(8), R.clique(3)], "ShmpTrunkSmallBackward")):
        torch.manual_seed(0)
        nm = NeighborhoodCountingModel(1, 64, neigh_args(dropout=p)).to_hetero_old(True, True).to(DEV)
        nm.train()
        names = _node_names(nm.emb_model_query(QueryBatch(graphs, DEV)))
        assert want in names and not ({"ShmpTrunkBackward", "ShmpTrunkSmallBackward"} - {want}) & names, (p, names)


def _neighborhood_batch():
    from helpers import golden_graphs
    from desco_amd.batch import NeighborhoodBatch
    from desco_amd.graphs import GraphSet
    from desco_amd.partition import build_partition
    part = build_partition(GraphSet.from_edge_lists(golden_graphs(max_n=41)[:10]), 4)
    return part, NeighborhoodBatch(part, DEV)


def _run_general_node(tag, case, batch, groups, has_anchor, drop):
    names = ["x0"] + (["aw", "ab"] if has_anchor else []) + [f"{k}{g}" for g in range(len(groups)) for k in ("wt", "bias")]
    vals = [case["x0"]] + (list(case["anchor"]) if has_anchor else []) + \
           [t for g in range(len(groups)) for t in (case["Wt"][g], case["bias"][g])]
    leaves = [t.clone().to(DEV).requires_grad_() for t in vals]
    pooled = AG.ShmpTrunk.apply(leaves[0], batch, groups, has_anchor, drop, *leaves[1:])
    fn = pooled.grad_fn
    xall, anch = torch.stack(fn.X[1:]), fn.anch
    (pooled * case["dpooled"].to(DEV)).sum().backward(retain_graph=True)
    grads = {"d" + n: t.grad for n, t in zip(names, leaves)}
    _gate_node(tag, "general node", case, pooled.detach(), grads, xall, anch)
    with pytest.raises(RuntimeError, match="ran twice"):
        (pooled * case["dpooled"].to(DEV)).sum().backward()


@pytest.mark.parametrize("x6", [True, False])
@pytest.mark.parametrize("p", [None, 0.2])
def test_general_node_matches_the_reference_on_a_neighborhood_batch(monkeypatch, x6, p):
    """autograd.ShmpTrunk on a NeighborhoodBatch (two row groups: count rows with 4 slots, canonical rows with 2; the
    anchor), fp32 mode, the layer products on the bf16x6 pipe and on the fp32 one, with layer dropout at sites 2 l + g;
    a second backward raises the documented RuntimeError."""
    monkeypatch.setattr(AG, "PRECISION", "fp32")
    monkeypatch.setattr(AG, "TRAIN_GEMM_BF16X6", x6)
    part, batch = _neighborhood_batch()
    Nc, N, B, L = batch.num_count, batch.num_rows, batch.num_graphs, 8
    case = R.neighborhood_case(part.vrowptr, part.vcol, part.count_ptr, N, L, 600)
    assert torch.equal(batch.vrowptr.cpu().long(), case["vrowptr"]) and case["groups"] == [(0, Nc, 4), (Nc, N, 2)]
    drop = None
    if p is not None:
        ops.manual_seed(77, step=5)
        drop = (ops.rng_next(DEV), p)
        case["factors"] = [torch.cat([ops.dropout_mask(ops.DropSite(drop[0], 2 * l, p), Nc, H),
                                      ops.dropout_mask(ops.DropSite(drop[0], 2 * l + 1, p), B, H)]).cpu() for l in range(L)]
    _run_general_node(f"ShmpTrunk neighborhood batch (N {N}, B {B}, L {L}), bf16x6 {x6}, dropout {p}", case, batch,
                      [("count", 0, Nc, 4), ("canonical", Nc, N, 2)], True, drop)


@pytest.mark.parametrize("layers", [1, 8])
def test_general_node_matches_the_reference_on_the_query_batch(monkeypatch, layers):
    """autograd.ShmpTrunk on the single-group query batch (no anchor, pooling over graph_ptr)"""
    from helpers import standard_queries
    monkeypatch.setattr(AG, "PRECISION", "fp32")
    graphs = standard_queries()[1]
    case = R.query_case(graphs, layers, "o1", 700 + layers)
    qb = _batch(graphs, case)
    _run_general_node(f"ShmpTrunk query batch, L {layers}", case, qb, [("union_node", 0, qb.num_rows, 2)], False, None)
