"""The gossip training trunks -- autograd.GossipTrunk with its fp32 backward and its bf16x6 one
(_gossip_trunk_backward_x6), and autograd.GossipTrunkDeep -- called directly on the operands of a case, every saved
activation and every returned gradient per element against the fp64 host reference tests/gossip_trunk_reference.py.
What the model-level gates (helpers.GOSSIP_GRAD_TOL: max |g - g_ref| / max |g_ref| <= 5e-3 per folded parameter) cannot
see is the chain: which operand feeds which launch, which dropout site and probability goes with which epilogue,
which block of wtp / wt_l is transposed into which slot, the slicing of the deep node's saved tensors, its chunked
copy2d_multi / linear_bwd_w_multi loops (both run twice at L = 9).

Gate (tests/test_shmp_trunk_kernels_gpu.py's; no number of its own): per tensor E_kernel = max |got - ref| / mag over
ALL elements, mag = the reference evaluated on absolute values (the sum of |terms| of the element).  E_kernel <= 4 E_f32,
where E_f32 is the same figure of the reference evaluated in float32 on the host on the same case, and E_kernel <= 1e-4.
Two families of few elements, each one sum over every row, take their factor from a host measurement instead of the 4
(gossip_trunk_reference.FACTOR: dg_l 7, db3 5): the kernels' reduction orders evaluated in fp32 on the host reach 6.2x
and 4.5x E_f32 without any kernel (test_the_column_sums_pass_the_factor_4_by_fp32_order_alone); the kernels measured
6.74x (dg1, 3 values, 237 nodes) and 4.59x (db3).
An element with mag == 0 must be exactly 0.  Two runs on the same inputs and key are bit-identical.
tests/test_gossip_trunk_reference_host.py proves the gate reachable (a second fp32 summation order stays within the
factor 4 on every case below) and that it catches six chain errors.

The forward is compared with the unpinned reference (relu is continuous).  The backward runs after that has passed,
and the reference backward pins relu' / leaky' to the node's own saved activations, so that a pre-activation within
rounding of zero does not become a discontinuous gradient difference.  Dropout: the factors the node applied are
exported with ops.dropout_mask from the node's own key and handed to the reference; (p_layer, p_post) differ.
Every test prints E_kernel, E_f32 and their ratio as ``[parity]`` lines; the worst ratio per form and tensor family is
printed once more when the module ends."""
import collections

import pytest
import torch

pytestmark = pytest.mark.gpu

import gossip_trunk_reference as R  # noqa: E402
from desco_amd import autograd as AG  # noqa: E402
from desco_amd import ops  # noqa: E402

DEV = "cuda"
H = R.H
CEILING = 1e-4
WORST = collections.defaultdict(float)          # "form, tensor family" -> worst E_kernel / E_f32 seen
_HOST = {}                                      # (case, drop) -> the unpinned host evaluations, shared by the forms


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    for k in sorted(WORST):
        print(f"[parity] gossip trunk worst E_kernel / E_f32 over the module, {k}: {WORST[k]:.2f} (gate {R.FACTOR[k.split(', ')[1]]})")


def _gate(name, got, ref, mag, f32, keys, form):
    """E_kernel <= 4 E_f32 (R.FACTOR: 7 for dg_l, 5 for db3, from the host's own fp32 orders) and <= CEILING for every
    tensor of ``keys``; zero where mag is zero"""
    bad = []
    for k in keys:
        assert tuple(got[k].shape) == tuple(ref[k].shape), (k, tuple(got[k].shape), tuple(ref[k].shape))
        g = got[k].detach().cpu().double()
        ek, i = R.scaled_error(g, ref[k], mag[k])
        ef, _ = R.scaled_error(f32[k], ref[k], mag[k])
        ratio = ek / ef if ef > 0 else (0.0 if ek == 0 else float("inf"))
        factor = R.FACTOR[R.family(k)]
        fam = f"{form}, {R.family(k)}"
        WORST[fam] = max(WORST[fam], ratio)
        print(f"[parity] {name} {k}: E_kernel {ek:.3e}, E_f32 {ef:.3e}, ratio {ratio:.2f} (gate {factor}, ceiling {CEILING:.0e})")
        exact = bool((g[mag[k] == 0] == 0).all())
        if not (ek <= factor * ef and ek <= CEILING and exact):
            bad.append(f"{name} {k}: E_kernel {ek:.3e} E_f32 {ef:.3e} ratio {ratio:.2f}; element {i}: got "
                       f"{float(g.flatten()[i])!r}, ref {float(ref[k].flatten()[i])!r}, mag {float(mag[k].flatten()[i])!r}"
                       f"{'' if exact else '; nonzero where mag == 0'}")
    assert not bad, "\n".join(bad)


def _bit_identical(name, a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{name} {k}: two runs on the same inputs differ"


# ---- one run of a node ------------------------------------------------------------------------------------------------
def _leaves(c, deep):
    """(the constant arguments, the names of the differentiable ones, their device leaves) in the node's order"""
    G, L = c["G"], c["L"]
    d = lambda t: t.to(DEV)                                                           # noqa: E731
    rowptr, col = torch.from_numpy(G.rowptr).to(DEV), torch.from_numpy(G.col).to(DEV)
    assert rowptr.dtype == torch.int32 and col.dtype == torch.int32 and col.numel() >= 1
    w3, w5 = d(c["w3t"].t().contiguous()), d(c["w5t"].t().contiguous())             # post_mp.3 / .5 as torch keeps them
    const = [rowptr, col, c["N"], c["Q"], d(c["C6"]), d(c["C3"]), d(c["C2"]), d(c["x"].reshape(-1))]
    if deep:
        names = ["V0", "w3t", "b3", "w5t", "b5", "w7", "b7", "wtp", "Vp"] + [f"{k}{l}" for l in range(1, L) for k in ("g", "wt", "V")]
    else:
        assert L == 2
        names = ["V0", "g1", "wt1", "V1", "wtp", "Vp", "w3t", "b3", "w5t", "b5", "w7", "b7"]
    val = lambda n: c[n] if n in c else c[n.rstrip("0123456789")][int(n[-1]) - 1]     # noqa: E731
    leaves = [val(n).clone().to(DEV).requires_grad_() for n in names]
    return const, w3, w5, names, leaves


def _forward(c, deep, drop, seed):
    """(pred, activations by the reference's names, the node's key, names, leaves) of one forward pass"""
    L, R_ = c["L"], c["R"]
    const, w3, w5, names, leaves = _leaves(c, deep)
    if drop is not None:
        ops.manual_seed(seed, step=3)
    if deep:
        pred = AG.GossipTrunkDeep.apply(*const, w3, w5, drop, L, *leaves)
        sv = pred.grad_fn.saved_tensors
        n0 = len(AG.GossipTrunkDeep.SAVED_HEAD)
        assert len(sv) == n0 + L + 3 * (L - 1)
        head = dict(zip(AG.GossipTrunkDeep.SAVED_HEAD, sv))
        acts = {f"h{l}": sv[n0 + l - 1] for l in range(1, L + 1)}
        acts.update({f"hh{l}": sv[n0 + L + l - 1] for l in range(1, L)})
        for l in range(1, L):                   # the tail of the saved list is what the backward takes it for
            assert torch.equal(sv[n0 + 2 * L - 1 + l - 1], leaves[names.index(f"g{l}")])
            assert torch.equal(sv[n0 + 3 * L - 2 + l - 1], leaves[names.index(f"wt{l}")])
    else:
        g1 = leaves[names.index("g1")]
        pred = AG.GossipTrunk.apply(*const, (1.0 - g1).detach().contiguous(), w3, w5, drop, *leaves)
        sv = pred.grad_fn.saved_tensors
        assert len(sv) == len(AG.GossipTrunk.SAVED)
        head = dict(zip(AG.GossipTrunk.SAVED, sv))
        acts = {"h1": head["h1"], "hh1": head["hh"], "h2": head["h2"]}
    acts.update(y=head["y"], y3=head["y3"], y5=head["y5"])
    for k, v in acts.items():
        assert tuple(v.shape) == (R_, 4 * H if k == "y5" else H) and v.dtype == torch.float32, (k, tuple(v.shape))
    assert tuple(pred.shape) == (R_,) and head["key"].numel() == (0 if drop is None else 2)
    acts = {k: v.detach().clone() for k, v in acts.items()}
    acts["pred"] = pred.detach().clone()
    return pred, acts, head["key"], names, leaves


def _backward(c, pred, names, leaves):
    pred.backward(c["dpred"].to(DEV))
    return {"d" + n: t.grad for n, t in zip(names, leaves)}


def _factors(c, key, drop):
    """the factors the node applied, from its own key: layer_site(l) with p_layer, SITE_POST with p_post"""
    L, R_ = c["L"], c["R"]
    assert AG.GossipTrunk.SITE_POST == R.SITE_POST and all(AG.GossipTrunk.layer_site(l) == R.layer_site(l) for l in range(1, 12))
    assert len({R.SITE_POST} | {R.layer_site(l) for l in range(1, L + 1)}) == L + 1
    fac = {f"h{l}": ops.dropout_mask(ops.DropSite(key, AG.GossipTrunkDeep.layer_site(l), drop[0]), R_, H).cpu()
           for l in range(1, L + 1)}
    fac["post"] = ops.dropout_mask(ops.DropSite(key, AG.GossipTrunk.SITE_POST, drop[1]), R_, H).cpu()
    for k, f in fac.items():
        p = drop[1] if k == "post" else drop[0]
        s = float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32))
        assert set(f.unique().tolist()) <= {0.0, s} and (p == 0 or R_ * H < 200 or abs(float((f != 0).float().mean()) - (1 - p)) < 0.05)
    return fac


def _check(tag, form, cname, c, deep, drop, seed):
    """forward against the unpinned reference, then backward against the reference pinned to the node's activations,
    then a second run bit for bit"""
    c = dict(c)
    L = c["L"]
    pred, acts, key, names, leaves = _forward(c, deep, drop, seed)
    if drop is not None:
        c["factors"] = _factors(c, key, drop)
        plain = _forward(c, deep, None, seed)[1]["pred"]
        assert float(((acts["pred"] - plain).abs() / (1 + plain.abs())).max()) > 1e-3, "the factors must matter"
        for l in range(1, L + 1):
            assert not acts[f"h{l}"].cpu()[c["factors"][f"h{l}"] == 0].any()
        assert not acts["y"].cpu()[c["factors"]["post"] == 0].any()
    hk = (cname, drop)
    if hk not in _HOST:
        _HOST[hk] = (c["factors"], R.evaluate(c, backward=False), R.mag(c, backward=False),
                     R.evaluate(c, torch.float32, backward=False))
    fac0, ref, m, f32 = _HOST[hk]
    assert drop is None or all(torch.equal(fac0[k], c["factors"][k]) for k in fac0), "one key, one set of factors"
    _gate(tag, acts, ref, m, f32, R.ACTIVATIONS(L), form)
    # backward on the node's own activations; the reference pinned to them
    grads = _backward(c, pred, names, leaves)
    assert set(grads) == set(R.GRADIENTS(L))
    pins = R.pins_of(acts)
    ref, m, f32 = R.evaluate(c, pins=pins), R.mag(c, pins), R.evaluate(c, torch.float32, pins=pins)
    _gate(tag, grads, ref, m, f32, R.GRADIENTS(L), form)
    pred2, acts2, _, names2, leaves2 = _forward(c, deep, drop, seed)
    _bit_identical(tag, acts, acts2)
    _bit_identical(tag, grads, _backward(c, pred2, names2, leaves2))
    return c, acts, grads


def _regime_asserts(c, acts, grads):
    if c["regime"] == "x1e6":           # a zero column of C: exactly 0, whatever the order of the sum
        assert float(c["x"].max()) > 9e5 and not c["x"][:, R.ZERO_Q].any()
        assert not grads["dV0"][R.ZERO_Q, 2:5].any() and not grads["dVp"][R.ZERO_Q, 0].any()
        assert grads["dV0"][R.ZERO_Q, :2].any() and grads["dVp"][R.ZERO_Q, 1].any()
    if c["regime"] == "deadrelu":       # whole columns dead on every row: whole columns of the gradients exactly 0
        D = R.DEAD_COLS
        assert not acts["h1"][:, D].any() and not acts["y3"][:, D].any() and not acts["y5"][:, D].any()
        for k, v in (("db3", grads["db3"][D]), ("dw3t", grads["dw3t"][:, D]), ("db5", grads["db5"][D]),
                     ("dw5t", grads["dw5t"][:, D]), ("dw7", grads["dw7"][D]), ("dV0", grads["dV0"][:, :, D]),
                     ("dwtp", grads["dwtp"][D]), ("dwt1", grads["dwt1"][D]), ("dwt1", grads["dwt1"][H:][D])):
            assert not v.any(), k
        assert grads["db3"].any() and grads["dV0"].any()
    if c["regime"] == "g1exact":
        assert (c["g"][0] == 0).any() and (c["g"][0] == 1).any() and grads["dg1"].cpu()[c["g"][0] == 0].any()


_TRUNK = [(name, drop, x6) for name, _, _, _, _, drops in R.TRUNK_CASES for drop in (None,) + tuple(drops)
          for x6 in (False, True)]


@pytest.mark.parametrize("name,drop,x6", _TRUNK, ids=[f"{n}, drop {d}, {'bf16x6' if x else 'fp32'}" for n, d, x in _TRUNK])
def test_gossip_trunk_matches_the_reference(monkeypatch, name, drop, x6):
    """autograd.GossipTrunk, fp32 mode, its products on the fp32 pipe (GossipTrunk.backward) and on the bf16x6 pipe
    (_gossip_trunk_backward_x6): one row with an empty CSR; the ladder at Q = 29 (isolated nodes, degrees to 33) with
    all three dropout settings; R no multiple of 128; 2000 nodes with a 1300-leaf star (two slabs of affine_rows_bwd,
    several blocks of colsum / rowdot_bwd partials); Q = 65 (the torch-folded caller's shape) and Q = 64; x to 1e6 with
    a zero column; gates at exact 0 and 1; dead columns."""
    assert {c[0] for c in R.TRUNK_CASES} >= {"one row", "ladder Q29", "hub Q5", "Q65 N40", "Q64 N20"}
    monkeypatch.setattr(AG, "PRECISION", "fp32")
    monkeypatch.setattr(AG, "TRAIN_GEMM_BF16X6", x6)
    c = R.trunk_case(name)
    seed = next(s for n, _, _, _, s, _ in R.TRUNK_CASES if n == name)
    form = "GossipTrunk bf16x6" if x6 else "GossipTrunk fp32"
    c, acts, grads = _check(f"{form}, {name} (N {c['N']}, Q {c['Q']}), dropout {drop}", form, name, c, False, drop, seed)
    _regime_asserts(c, acts, grads)


_DEEP = [(name, drop) for name, _, _, drops in R.DEEP_CASES for drop in (None,) + tuple(drops)]


@pytest.mark.parametrize("name,drop", _DEEP, ids=[f"{n}, drop {d}" for n, d in _DEEP])
def test_gossip_trunk_deep_matches_the_reference(monkeypatch, name, drop):
    """autograd.GossipTrunkDeep at L = 1, 2, 3 and 9 on the ladder with Q = 3: at L = 9 the backward makes 25 copies
    (copy2d_multi takes 24 per launch) and 19 weight-gradient problems (linear_bwd_w_multi takes 16), so both chunk
    loops run twice; L = 3 with both dropout settings (sites 0, 1, 3 and post_mp.1 = 2)."""
    assert {c[1] for c in R.DEEP_CASES} >= {1, 2, 3, 9} and 3 * 9 - 2 > 24 and 2 * 9 + 1 > 16
    monkeypatch.setattr(AG, "PRECISION", "fp32")
    c = R.deep_case(name)
    seed = next(s for n, _, s, _ in R.DEEP_CASES if n == name)
    _check(f"GossipTrunkDeep, {name} (L {c['L']}), dropout {drop}", "GossipTrunkDeep", name, c, True, drop, seed)


@pytest.mark.parametrize("drop", [None, R.DROPS[1]], ids=["drop None", f"drop {R.DROPS[1]}"])
def test_gossip_trunk_on_the_deep_nodes_case_at_two_layers(monkeypatch, drop):
    """L = 2 is both nodes' ground: GossipTrunk (fp32 pipe) on the case GossipTrunkDeep runs at L = 2.  Each is held
    to the fp64 reference (the one shared between them here); they are not compared bit for bit."""
    monkeypatch.setattr(AG, "PRECISION", "fp32")
    monkeypatch.setattr(AG, "TRAIN_GEMM_BF16X6", False)
    c = R.deep_case("deep L2")
    seed = next(s for n, _, s, _ in R.DEEP_CASES if n == "deep L2")
    _check(f"GossipTrunk fp32, deep L2 case, dropout {drop}", "GossipTrunk fp32", "deep L2", c, False, drop, seed)
