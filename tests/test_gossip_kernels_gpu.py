"""The gossip kernels of the inference pass, each launched through its ``ops`` wrapper on synthetic operands and compared
element by element with the fp64 host reference of tests/gossip_reference.py (never through a model):

  * desco_gossip_scalars_f32 alone: |got - ref| <= tau * mag (the rule of tests/test_train_kernels_gpu.py), both lane
    mappings and their edges, strided x, exact gates;
  * desco_gossip_fused_f16x3_f32 (the product path) and desco_gossip_fused_f32 (bf16x6), with and without a tile order,
    from records the HOST computed: E = max |got - ref64| / D with D = |x| + |b7| + sum_c |y3[c] w7[c]| (the sum of
    absolute terms of the last dot product).  The kernels claim fp32 accuracy, so the gate is E_kernel <= 4 E_f32, E_f32
    being the error of the reference function evaluated at float32 on the CPU in the same test -- never a constant taken
    from a kernel.  (Two fp32 summation orders of the formula differ by 0.57-0.93x, tests/test_gossip_reference_host.py;
    a weight plane dropped in 16 k columns of one block lands at 90-290x.)  The reference uses the fp32 weight matrices
    handed to the split functions, so a wrong split or weight-stream permutation shows;
  * what needs no tolerance, bit for bit: tile order given or not, a launch over a slice of the queries, a graph alone
    or inside a larger batch, the ``out=`` destination and the queue words, desco_gossip_tile_order's permutation;
  * desco_gossip_layer_f16x3_f32 (depth != 2) against fp64 from the fp32 weights, |got - ref| <= 1e-5 * mag.

Every test prints one ``[parity]`` line with its worst error / bound."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from desco_amd import ops  # noqa: E402

import gossip_reference as R  # noqa: E402
from test_train_kernels_gpu import _bitequal, _bounded, _tau  # noqa: E402

DEV = "cuda"
ROW_CAP = 500_000           # (node, query) rows per case: keeps the fp64 reference a matter of seconds
GATE = 4.0                  # E_kernel <= GATE * E_f32


# ---- graphs ---------------------------------------------------------------------------------------------------------
def _ticket_copies():
    """copies of the ladder for a batch whose work units outnumber the resident waves 3:1 at Q = 29, so that waves draw
    tickets from the queue: ceil(N / 16) * ceil(29 / 5) >= 3 * 8 * multiprocessors"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_min = 16 * -(-3 * 8 * cus // 6)
    return -(-n_min // R.ladder_edges()[0]), cus


@functools.lru_cache(maxsize=None)
def _graph(name):
    lad = R.ladder_edges()
    if name == "ladder":
        g = lad
    elif name == "ladder_perm":
        g = R.permuted(*lad, seed=7)
    elif name == "hub":
        g = R.hub_edges()
    elif name.startswith("prefix"):
        g = R.prefix(int(name[6:]), lad[1])
    elif name == "n256":                              # two whole 128-node tiles
        g = R.concat([lad, R.prefix(19, lad[1])])
    elif name == "tickets":
        g = R.concat([lad] * _ticket_copies()[0])
    else:
        raise KeyError(name)
    G = R.Graph(*g)
    G.rowptr_dev = torch.from_numpy(G.rowptr).to(DEV)
    G.col_dev = torch.from_numpy(G.col).to(DEV)
    G.tile_perm = ops.gossip_tile_order(G.rowptr_dev, G.n)
    return G


def test_the_test_graphs_have_the_shapes_they_are_meant_to_have():
    lad, perm, hub = _graph("ladder"), _graph("ladder_perm"), _graph("hub")
    for G in (lad, perm):
        count = np.bincount(G.deg)
        assert G.n == 237 and all(count[d] == d + 1 for d in list(range(18)) + [31, 33]) and count.sum() == 237
    lo = np.bincount(lad.src[lad.dst < lad.src].numpy(), minlength=lad.n)
    assert ((lo > 0) & (lo < lad.deg)).sum() == 237 - 2 * 19 - 1  # all but a clique's ends: neighbours on both sides of the id
    assert not np.array_equal(lad.deg, perm.deg)
    assert hub.deg.max() == R.STAR_LEAVES > 1216 and (hub.deg == 0).sum() > 400     # > one staging pass of bf16x6
    g16 = hub.deg[:hub.n // 16 * 16].reshape(-1, 16)
    assert ((g16.max(1) > 1000) & (g16.min(1) == 0)).any()       # one long row among empty ones in a wave group
    copies, cus = _ticket_copies()
    n = copies * 237
    assert -(-n // 16) * 6 >= 3 * 8 * cus and n * 29 <= ROW_CAP, (n, cus)
    print(f"[parity] gossip test graphs: ladder 237 nodes (degrees 0-17, 31, 33), hub set {hub.n} nodes (max degree "
          f"{hub.deg.max()}), ticket batch {n} nodes for {cus} CUs (error / bound = 0)")


# ---- operands on the device -----------------------------------------------------------------------------------------
class Case:
    """graph + operand regime + query count: host operands, host records scal4 [N, Q, 4] (fp64 formula rounded to fp32)
    and the device operand sets of both kernel forms"""

    def __init__(self, graph, Q, regime, seed):
        self.name = f"{graph} Q={Q} {regime}"
        self.G, self.Q, self.regime = _graph(graph), Q, regime
        assert self.G.n * Q <= ROW_CAP
        self.P = R.operands(Q, regime, seed)
        self.x = R.features(self.G.n, Q, regime, seed)
        self.scal4 = R.scalars(self.x, self.G, self.P["g0"], self.P["g1"])[0].float()
        d = {k: v.to(DEV) for k, v in self.P.items() if isinstance(v, torch.Tensor)}
        self.v = {k: d[k] for k in ("g1", "p", "z", "zp", "r", "t", "u", "tp", "d1", "b3", "b5", "w7")}
        self.v["b7"] = self.P["b7"]
        for k in ("w1", "wp", "w3", "w5"):
            self.v[k + "s"] = ops.split_bf16_planes(d[k])
        self.v["wstream"], self.v["winv"] = ops.gossip_f16_stream(*[ops.split_f16_planes(d[k])
                                                                    for k in ("w1", "wp", "w3", "w5")])
        self.scal_dev = self.scal4.to(DEV)

    def reference(self):
        """(ref64 [N, Q], D, E_f32), computed once; asserts that the case is not degenerate"""
        if not hasattr(self, "_ref"):
            ref, D, stats = R.net(self.scal4, self.G, self.P)
            f32, _, _ = R.net(self.scal4, self.G, self.P, torch.float32)
            e32, _ = R.scaled_error(f32, ref, D)
            assert torch.isfinite(ref).all() and torch.isfinite(D).all() and (D > 0).all(), self.name
            corr = ref - self.x.double()
            if self.regime == "zeros":
                assert e32 == 0 and stats["h1_zero"] == 1 and (ref == float(np.float32(self.P["b7"]))).all()
            else:
                assert 0 < e32 < 1e-5, (self.name, e32)           # (a handful of fp32 roundings: 1e-7, 2e-6 on hub rows)
                if self.Q > 1:
                    assert float((corr.max(1).values - corr.min(1).values).max()) > 1e-3 * float(corr.abs().max())
                assert float(corr.abs().max()) > 0
            if self.regime == "deadrelu":                        # whole h1 / h2 vectors of many rows exactly zero
                assert 0.05 <= stats["h1_zero"] <= 0.95 and 0.05 <= stats["h2_zero"] <= 0.95, (self.name, stats)
            elif self.regime != "zeros":
                assert stats["h1_zero"] < 0.05 and stats["h2_zero"] < 0.05, (self.name, stats)
            if self.regime == "halfzero":
                assert 0.4 <= float((self.x == 0).all(1).float().mean()) <= 0.6 or self.G.n < 4
            if self.regime == "g1exact" and self.Q >= 3:
                assert (self.P["g1"] == 0).any() and (self.P["g1"] == 1).any()
            self.stats = stats
            self._ref = (ref, D, e32)
        return self._ref

    def launch(self, form, tiled, q0=0, q1=None, G=None, scal=None, out=None, queue=None):
        """one launch of the fused kernel ``form`` over queries [q0, q1) on graph G (default: the case's own)"""
        G = G or self.G
        q1 = self.Q if q1 is None else q1
        whole = q0 == 0 and q1 == self.Q
        v = dict(self.v)
        if not whole:
            for k in ("g1", "p", "z", "zp"):
                v[k] = v[k][q0:q1].contiguous()
        scal = self.scal_dev if scal is None else scal
        if not whole:
            scal = scal[:, q0:q1].contiguous()
        scal = scal.reshape(-1, 4)
        tperm = G.tile_perm if tiled else None
        if form == "bf16x6":
            assert out is None
            return ops.gossip_fused(scal, G.rowptr_dev, G.col_dev, G.n, q1 - q0, v, tile_perm=tperm)
        queue = torch.zeros(2, dtype=torch.int64, device=DEV) if queue is None else queue
        got = ops.gossip_fused_f16(scal, G.rowptr_dev, G.col_dev, G.n, q1 - q0, v, queue, tile_perm=tperm, out=out)
        assert int(queue.abs().sum()) == 0, "the kernel must leave its queue words zero"
        return got


@functools.lru_cache(maxsize=2)
def _case(graph, Q, regime, seed):
    return Case(graph, Q, regime, seed)


# ---- desco_gossip_scalars_f32 ---------------------------------------------------------------------------------------
def _scalars_graph(N):
    """degrees 0-9 with tails of 1, 2, 3 neighbours after full steps of four; at N = 1001 a hub row as well"""
    rng = np.random.default_rng(N)
    if N <= 9:
        edges = [(a, b) for a in range(N) for b in range(a + 1, N) if rng.random() < 0.6 and a != 3]   # id 3: isolated
        return R.Graph(N, edges)
    cliques = R.concat([(k, [(a, b) for a in range(k) for b in range(a + 1, k)]) for k in range(1, 11)])      # 55 ids
    n, edges = cliques
    edges = edges + [(int(rng.integers(55, v)), v) for v in range(56, N - 1) if rng.random() < 0.8]
    edges += [(N - 1, v) for v in range(100, N - 1, 2)] + [(500, v) for v in range(0, N - 1, 4) if v != 500]
    return R.Graph(N, edges)


@pytest.mark.parametrize("N", [1, 2, 7, 8, 9, 1001])
@pytest.mark.parametrize("Q", [1, 2, 31, 32, 33, 63, 64])
def test_gossip_scalars_against_fp64(Q, N):
    G = _scalars_graph(N)
    if N == 1001:
        assert set(range(10)) <= set(G.deg.tolist()) and G.deg.max() > 167
        assert all(((G.deg > 4) & (G.deg % 4 == r)).any() for r in (1, 2, 3))
    g = torch.Generator().manual_seed(1000 * Q + N)
    wide = torch.rand(N, Q + 5, generator=g) * 30
    wide[torch.arange(N) % 3 == 2] = 0                                    # rows of x = 0
    g0, g1 = torch.rand(Q, generator=g), torch.rand(Q, generator=g)
    for i, val in enumerate((0.0, 1.0, 0.5)):                             # exact gates among random ones
        if i < Q:
            g0[i] = val
            g1[(i + 1) % Q] = val
    wide_dev = wide.to(DEV)
    x_dev = wide_dev[:, 2:2 + Q]                                          # a column slice: ldx = Q + 5
    assert not x_dev.is_contiguous() or N == 1
    got = ops.gossip_scalars(x_dev, torch.from_numpy(G.rowptr).to(DEV), torch.from_numpy(G.col).to(DEV),
                             g0.to(DEV), g1.to(DEV)).cpu().view(N, Q, 4)
    x = wide[:, 2:2 + Q]
    ref, mag = R.scalars(x, G, g0, g1)
    assert torch.isfinite(got).all()
    _bitequal(f"gossip_scalars Q={Q} N={N} x", got[..., 3].contiguous(), x.contiguous())
    # a row's sums run over its lower / higher neighbours one after the other: chain = the longer of the two
    lo = np.bincount(G.src[G.dst < G.src].numpy(), minlength=N)
    chain = np.maximum(lo, G.deg - lo)
    long_rows = torch.from_numpy(chain > 167)
    for rows, tau, tag in ((~long_rows, _tau(int(chain[chain <= 167].max(initial=1))), "rows of <= 167 terms"),
                           (long_rows, _tau(int(chain.max(initial=1))), "hub rows")):
        if rows.any():
            _bounded(f"gossip_scalars Q={Q} N={N} (a0, b0, a1), {tag}", got[rows][..., :3], ref[rows][..., :3],
                     mag[rows][..., :3], tau)
    if Q > 1 and N > 1:
        assert (ref[..., 0] != ref[..., 2]).any()                         # g0 != g1: a0 and a1 cannot stand in for each other


# ---- the fused kernels against fp64 ---------------------------------------------------------------------------------
def _fused_cases():
    cases = [(g, 29, reg) for g in ("ladder", "ladder_perm", "hub") for reg in R.REGIMES]
    qs = (1, 4, 5, 6, 64, 65, 100)
    cases += [("ladder_perm", q, R.REGIMES[i % len(R.REGIMES)]) for i, q in enumerate(qs)]
    cases += [("ladder", q, R.REGIMES[(i + 3) % len(R.REGIMES)]) for i, q in enumerate(qs)]
    cases += [("ladder", 5, "zeros"), ("hub", 6, "x1e-3"), ("hub", 64, "deadrelu"), ("hub", 5, "wscales")]
    # the small sizes: few nodes take many queries, so that the worst of a case is a worst of >= 100 elements ("deadrelu"
    # wants degrees above 10 for live rows: the three larger prefixes only)
    small = {1: ((100, "o1"), (65, "rows2^18")), 15: ((29, "x1e6"), (64, "wscales")), 16: ((65, "x1e-3"), (6, "halfzero")),
             17: ((100, "rows2^18"), (5, "g1exact")), 127: ((4, "wscales"), (29, "deadrelu")),
             128: ((5, "halfzero"), (64, "deadrelu")), 129: ((6, "g1exact"), (1, "x1e6"))}
    for n, pairs in small.items():
        cases += [(f"prefix{n}", q, reg) for q, reg in pairs]
    cases += [("tickets", 29, "o1")]
    return [c + (seed,) for seed, c in enumerate(cases)]


FUSED_CASES = _fused_cases()
FUSED_PARAMS = [c + (form, tiled) for c in FUSED_CASES for form in ("f16x3", "bf16x6") for tiled in (False, True)]
WORST = {}


def _where(G, Q, i):
    node, q = divmod(i, Q)
    return (f"node {node} query {q} degree {int(G.deg[node])} lane group slot {node % 16} group {node // 16} "
            f"unit {q // 5}")


@pytest.mark.parametrize("graph,Q,regime,seed,form,tiled", FUSED_PARAMS,
                         ids=[f"{g}-Q{q}-{r}-{f}-{'tiled' if t else 'plain'}" for g, q, r, _, f, t in FUSED_PARAMS])
def test_fused_gossip_is_fp32_accurate(graph, Q, regime, seed, form, tiled):
    c = _case(graph, Q, regime, seed)
    ref, D, e32 = c.reference()
    got = c.launch(form, tiled).cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all(), c.name
    e, i = R.scaled_error(got, ref, D)
    ratio = e / e32 if e32 > 0 else (0.0 if e == 0 else float("inf"))
    print(f"[parity] gossip fused {form} {'tile order' if tiled else 'node order'} {c.name} ({c.G.n} nodes): "
          f"E_kernel {e:.3e}, E_f32 {e32:.3e}, worst error / bound = {ratio / GATE:.3e} (ratio {ratio:.2f}, gate {GATE:.0f}; "
          f"zero h1 / h2 rows {c.stats['h1_zero']:.2f} / {c.stats['h2_zero']:.2f})")
    WORST[form] = max(WORST.get(form, (0.0, "")), (ratio, c.name))
    assert ratio <= GATE, (f"{c.name} {form}: E_kernel {e:.3e} > {GATE:.0f} x E_f32 {e32:.3e} at {_where(c.G, Q, i)}: got "
                           f"{float(got.flatten()[i])!r}, ref {float(ref.flatten()[i])!r}, D {float(D.flatten()[i])!r}")


def test_fused_gossip_worst_ratio_per_form():
    """the figure DESIGN.md section 2 quotes (runs after the cases above; under -k it reports what ran)"""
    for form, (ratio, name) in sorted(WORST.items()):
        print(f"[parity] gossip fused {form}: worst E_kernel / E_f32 over {len(FUSED_CASES)} cases x 2 orders = "
              f"{ratio:.2f} ({name}); worst error / bound = {ratio / GATE:.3e}")
        assert ratio <= GATE


# ---- bit-equal invariants -------------------------------------------------------------------------------------------
ALL_GRAPHS = ["ladder", "ladder_perm", "hub", "n256", "tickets"] + [f"prefix{n}" for n in (1, 15, 16, 17, 127, 128, 129)]


@pytest.mark.parametrize("form", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("graph", ALL_GRAPHS)
def test_tile_order_changes_no_bit(graph, form):
    Q = 29 if graph == "tickets" else 7
    c = _case(graph, Q, "o1", 100)
    a, b = c.launch(form, True), c.launch(form, False)
    assert float(a.abs().max()) > 0
    _bitequal(f"gossip fused {form} {c.name}: tile order vs node order", a, b)


@pytest.mark.parametrize("N", [1, 127, 128, 129, 256])
def test_gossip_tile_order_at_tile_edges(N):
    G = _graph("n256" if N == 256 else f"prefix{N}")
    assert G.n == N and (N < 100 or len(set(G.deg.tolist())) >= 14)       # many ties, many degrees
    perm = G.tile_perm.cpu().numpy()
    assert perm.shape == (-(-N // 128) * 128,)
    R.check_tile_order(perm, G.rowptr, N)
    print(f"[parity] gossip_tile_order N={N}: the stable degree order in snake slots, padded slots last "
          f"(error / bound = 0)")


@pytest.mark.parametrize("form,tiled", [("f16x3", False), ("f16x3", True), ("bf16x6", False)])
def test_a_launch_over_a_slice_of_the_queries_changes_no_bit(form, tiled):
    """what the product relies on when it splits more than 64 queries, and what a one-query-ahead prefetch across a
    unit boundary would break: cuts at 1, 4, 5, 6 and 64"""
    c = _case("ladder_perm", 100, "o1", 101)
    whole = c.launch(form, tiled)
    cuts = [0, 1, 4, 5, 6, 64, 100]
    for q0, q1 in list(zip(cuts[:-1], cuts[1:])) + [(1, 6), (4, 64), (5, 100), (0, 64)]:
        part = c.launch(form, tiled, q0, q1)
        _bitequal(f"gossip fused {form} {'tiled' if tiled else 'plain'} queries [{q0}:{q1}] of 100",
                  part, whole[:, q0:q1].contiguous())


@pytest.mark.parametrize("form", ["f16x3", "bf16x6"])
def test_a_graph_alone_or_inside_a_batch_changes_no_bit(form):
    """rows of a graph launched alone equal its rows in a batch where it sits behind and in front of other graphs (ids
    shifted by 17 and 254: its nodes fall into other 16-node groups and 128-node tiles)"""
    Q, names = 29, ["prefix17", "ladder", "ladder_perm", "prefix129"]
    c = _case("ladder", Q, "o1", 102)
    parts = [_graph(n) for n in names]
    union = R.Graph(*R.concat([(G.n, G.edges) for G in parts]))
    union.rowptr_dev, union.col_dev = torch.from_numpy(union.rowptr).to(DEV), torch.from_numpy(union.col).to(DEV)
    xs = [R.features(G.n, Q, "o1", 200 + i) for i, G in enumerate(parts)]
    scals = [R.scalars(x, G, c.P["g0"], c.P["g1"])[0].float().to(DEV) for x, G in zip(xs, parts)]
    both = R.scalars(torch.cat(xs), union, c.P["g0"], c.P["g1"])[0].float().to(DEV)
    assert torch.equal(both, torch.cat(scals))                    # (the records of a node depend on its own graph only)
    got = c.launch(form, False, G=union, scal=both)
    n0 = 0
    for G, s, name in zip(parts, scals, names):
        alone = c.launch(form, False, G=G, scal=s)
        _bitequal(f"gossip fused {form} {name} alone vs rows {n0}.. of a {union.n}-node batch", alone,
                  got[n0:n0 + G.n].contiguous())
        n0 += G.n


@pytest.mark.parametrize("graph,tiled", [("prefix129", False), ("prefix129", True), ("prefix17", False), ("prefix1", True)])
def test_out_destination_and_queue(graph, tiled):
    """``out=``: exactly N * Q floats are written (the rows past N of the ragged last group / tile do not exist for the
    kernel); the queue words are zero after every launch and two launches sharing a queue agree"""
    Q = 7
    c = _case(graph, Q, "o1", 103)
    n, pad = c.G.n * Q, 256
    plain = c.launch("f16x3", tiled)
    sentinel = torch.full((n + 2 * pad,), -12345.0, device=DEV)
    buf = sentinel.clone()
    queue = torch.zeros(2, dtype=torch.int64, device=DEV)
    got = c.launch("f16x3", tiled, out=buf[pad:pad + n].view(c.G.n, Q), queue=queue)
    assert got.data_ptr() == buf[pad:].data_ptr()
    again = c.launch("f16x3", tiled, queue=queue)
    _bitequal(f"gossip fused f16x3 {c.name} out= vs its own buffer", got, plain)
    _bitequal(f"gossip fused f16x3 {c.name} second launch on a shared queue", again, plain)
    _bitequal(f"gossip fused f16x3 {c.name} floats around out=", torch.cat([buf[:pad], buf[pad + n:]]),
              torch.cat([sentinel[:pad], sentinel[pad + n:]]))


# ---- desco_gossip_layer_f16x3_f32 -----------------------------------------------------------------------------------
def _layer_graph(name):
    if name != "syn_hub":
        return _graph(name)
    from test_gossip_depth_gpu import syn_hub_graphs          # the shape the one-shape fp64 check of that file ran on
    G = R.Graph(*R.concat(syn_hub_graphs().edge_lists()))
    G.rowptr_dev, G.col_dev = torch.from_numpy(G.rowptr).to(DEV), torch.from_numpy(G.col).to(DEV)
    return G


LAYER_CASES = [("prefix1", 1), ("prefix1", 29), ("prefix1", 70), ("prefix9", 7), ("prefix65", 1), ("prefix127", 1),
               ("prefix128", 29), ("ladder", 29), ("ladder", 70), ("ladder_perm", 1), ("hub", 29), ("syn_hub", 29)]


@pytest.mark.parametrize("with_pn", [True, False])
@pytest.mark.parametrize("graph,Q", LAYER_CASES)
def test_gossip_layer_against_fp64(graph, Q, with_pn):
    """One gossip layer l >= 1: out = relu([hh | h] W + c3 . v[q]), acc += h P (+ out Pn), the reference in fp64 from the
    fp32 weights handed to split_f16_planes; mag = the formula on absolute values, one stage for out, two for acc."""
    G = _layer_graph(graph)
    N, R_ = G.n, G.n * Q
    if graph in ("prefix9", "prefix127"):
        assert R_ % 64 == 63
    elif graph in ("prefix65",) or (graph, Q) == ("prefix1", 1):
        assert R_ % 64 == 1
    elif graph == "prefix128":
        assert R_ % 64 == 0
    g = torch.Generator().manual_seed(11 + R_)
    h = torch.rand(R_, 64, generator=g)
    h[torch.rand(R_, generator=g) < 0.1] = 0
    gate = torch.rand(Q, generator=g)
    c3 = torch.rand(R_, 3, generator=g)
    v = torch.randn(Q, 3, 64, generator=g) * 0.1
    W, P, Pn = (torch.randn(64, 128, generator=g) * 0.05, torch.randn(64, 64, generator=g) * 0.1,
                torch.randn(64, 64, generator=g) * 0.1)
    acc0 = torch.randn(R_, 64, generator=g)
    acc = acc0.to(DEV)
    out = ops.gossip_layer_f16(h.to(DEV), G.rowptr_dev, G.col_dev, N, Q, gate.to(DEV), c3.to(DEV), v.to(DEV),
                               ops.split_f16_planes(W.to(DEV)), ops.split_f16_planes(P.to(DEV)), acc,
                               pn=ops.split_f16_planes(Pn.to(DEV)) if with_pn else None)
    assert torch.isfinite(out).all() and torch.isfinite(acc).all()

    def formula(hq, accq, Wq, Pq, c3q, vq):
        hq = hq.view(N, Q, 64)
        wgt = torch.where((G.dst < G.src)[:, None], gate.double()[None, :], 1 - gate.double()[None, :])     # [E, Q]
        hh = torch.zeros_like(hq).index_add_(0, G.src, wgt[..., None] * hq[G.dst])
        o = torch.cat([hh, hq], -1).view(R_, 128) @ Wq.t() + (c3q[:, :, None] * vq[torch.arange(R_) % Q]).sum(1)
        return o, accq + hq.view(R_, 64) @ Pq.t()

    d = lambda t: t.double()                                                          # noqa: E731
    pre, ref_acc = formula(d(h), d(acc0), d(W), d(P), d(c3), d(v))
    ref = pre.clamp_min(0)
    mag, mag_acc = formula(d(h).abs(), d(acc0).abs(), d(W).abs(), d(P).abs(), d(c3).abs(), d(v).abs())
    if with_pn:
        ref_acc = ref_acc + ref @ d(Pn).t()
        mag_acc = mag_acc + mag @ d(Pn).abs().t()
    assert float((ref == 0).float().mean()) < 0.9 and float(ref.max()) > 0
    tag = f"gossip_layer {graph} Q={Q} R={R_} (R % 64 = {R_ % 64}) pn={'given' if with_pn else 'None'}"
    _bounded(tag + " out", out, ref, mag, 1e-5)
    _bounded(tag + " acc", acc, ref_acc, mag_acc, 1e-5)
