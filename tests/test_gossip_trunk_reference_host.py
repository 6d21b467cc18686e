"""tests/gossip_trunk_reference.py on the host, before any GPU is involved:
  * the reference against a dense evaluation of the same contract (a lower and an upper 0/1 adjacency matrix, no
    ``index_add_``) on 10 nodes, Q = 3, L = 1, 2, 3 with dropout factors, and its written-out backward against torch
    autograd of that dense forward in fp64, so that it is not its own only witness; the pin convention (act'(c) from
    the activation output, c > 0) reproduces the unpinned evaluation from its own activations;
  * its constants C6 / C3 / C2 and its CSR against the product's host-visible batch (GossipBatch on the host) and
    against gossip_reference.scalars, stacked as gnn_model.gossip_forward_train stacks them;
  * the gate of tests/test_gossip_trunk_kernels_gpu.py (E_kernel <= 4 E_f32 on the scale ``mag``) is reachable by a
    correct fp32 implementation: a second fp32 summation order stays within 4x the fp32 evaluation's error on every
    tensor of every case that file runs, and E_f32 > 0 wherever the tensor has a term to round;
  * the gate catches chain errors: six known wrong chains, evaluated in fp64 in the reference itself, each exceed the
    1e-4 ceiling on every tensor they touch; the factor over the ceiling is printed;
  * the 9-layer case keeps every layer alive."""
import pytest
import torch

import gossip_reference as GR
import gossip_trunk_reference as R

H = R.H
CEILING = 1e-4


# ---- dense witness ----------------------------------------------------------------------------------------------------
def _witness(L):
    """10 nodes: a 5-clique, a path, a node with neighbours on both sides only, an isolated node; Q = 3; factors"""
    edges = [(a, b) for a in range(5) for b in range(a + 1, 5)] + [(4, 5), (5, 6), (6, 7), (2, 8), (8, 7)]
    c = R.case((10, edges), 3, L, "o1", 40 + L)
    c["factors"] = R.bernoulli_factors(c, (0.3, 0.1), 50 + L)
    A = torch.zeros(10, 10, dtype=torch.float64)
    for a, b in edges:
        A[a, b] = A[b, a] = 1
    return c, torch.tril(A, -1), torch.triu(A, 1)


def _dense(c, Alo, Ahi):
    """the contract with matrices and torch autograd, fp64; the constants from the matrices as well"""
    N, Q, L = c["N"], c["Q"], c["L"]
    d = lambda t: t.double().clone().requires_grad_()                                 # noqa: E731
    x = c["x"].double()
    dlo, dhi, slo, shi = Alo.sum(1, keepdim=True).expand(N, Q), Ahi.sum(1, keepdim=True).expand(N, Q), Alo @ x, Ahi @ x
    one = torch.ones(N, Q, dtype=torch.float64)
    C6 = torch.stack([dhi, dlo - dhi, shi, slo - shi, x, one], -1)
    C3, C2 = torch.stack([dhi, dlo - dhi, one], -1), torch.stack([x, one], -1)
    C6, C3, C2 = (C.float().double() for C in (C6, C3, C2))       # rounded once to the fp32 operands, as the case's are
    P = {k: d(c[k]) for k in ("V0", "Vp", "wtp", "w3t", "b3", "w5t", "b5", "w7", "b7")}
    g, wt, V = [d(t) for t in c["g"]], [d(t) for t in c["wt"]], [d(t) for t in c["V"]]
    f = lambda k: c["factors"][k].double().view(N, Q, H)                              # noqa: E731
    aff = lambda C, Vq: torch.einsum("nqk,qkc->nqc", C, Vq)                            # noqa: E731
    h = [None, f("h1") * torch.relu(aff(C6, P["V0"]))]
    hh = [None]
    for l in range(1, L):
        gl = g[l - 1][None, :, None]
        hh.append(gl * torch.einsum("ij,jqc->iqc", Alo, h[l]) + (1 - gl) * torch.einsum("ij,jqc->iqc", Ahi, h[l]))
        h.append(f(f"h{l + 1}") * torch.relu(torch.cat([hh[l], h[l]], -1) @ wt[l - 1] + aff(C3, V[l - 1])))
    y = f("post") * torch.nn.functional.leaky_relu(torch.cat(h[1:], -1) @ P["wtp"] + aff(C2, P["Vp"]), 0.1)
    y3 = torch.relu(y @ P["w3t"] + P["b3"])
    y5 = torch.relu(y3 @ P["w5t"] + P["b5"])
    pred = x + P["b7"] + y5 @ P["w7"]
    pred.backward(c["dpred"].double().view(N, Q))
    out = {f"h{l}": h[l] for l in range(1, L + 1)}
    out.update({f"hh{l}": hh[l] for l in range(1, L)})
    out.update(y=y, y3=y3, y5=y5, pred=pred, dV0=P["V0"].grad, dwtp=P["wtp"].grad, dVp=P["Vp"].grad, dw3t=P["w3t"].grad,
               db3=P["b3"].grad, dw5t=P["w5t"].grad, db5=P["b5"].grad, dw7=P["w7"].grad, db7=P["b7"].grad)
    for l in range(1, L):
        out[f"dg{l}"], out[f"dwt{l}"], out[f"dV{l}"] = g[l - 1].grad, wt[l - 1].grad, V[l - 1].grad
    consts = dict(C6=C6.reshape(-1, 6), C3=C3.reshape(-1, 3), C2=C2.reshape(-1, 2))
    return {k: v.detach() for k, v in out.items()}, consts


@pytest.mark.parametrize("L", [1, 2, 3])
def test_reference_equals_the_dense_formula_and_torch_autograd(L):
    c, Alo, Ahi = _witness(L)
    want, consts = _dense(c, Alo, Ahi)
    for k, v in consts.items():
        assert torch.equal(v.float(), c[k]), k                     # (sums of at most 5 fp32 values: exact in fp64)
    got, m = R.evaluate(c), R.mag(c)
    assert set(got) == set(want) == set(R.ACTIVATIONS(L) + R.GRADIENTS(L))
    for k in want:
        e, _ = R.scaled_error(got[k], want[k].reshape(got[k].shape), m[k])
        print(f"[parity] gossip trunk reference vs dense formula + autograd, L {L} {k}: max |d| / mag = {e:.2e}")
        assert e <= 1e-13, k
        assert (m[k] >= got[k].abs() * (1 - 1e-12)).all(), k       # the sum of |terms| bounds the sum
    # pinned to its own activations the reference is the unpinned one (the convention act'(c) = c > 0 on the output)
    pinned = R.evaluate(c, pins=R.pins_of(got))
    for k in got:
        assert torch.equal(pinned[k], got[k]) or R.scaled_error(pinned[k], got[k], m[k])[0] <= 1e-15, k
    # the witness exercises what it claims: both sides of a node, an isolated node, live and dropped elements
    assert (Alo.sum(1) > 0).any() and (Ahi.sum(1) > 0).any() and ((Alo + Ahi).sum(1) == 0).any()
    if L > 1:
        assert (got["hh1"].view(10, 3, H)[9] == 0).all() and (m["hh1"].view(10, 3, H)[9] == 0).all()
        assert (got["dg1"].abs() > 1e-3).all()


def test_pin_convention_is_the_librarys_act_grad():
    """relu'(c) = (c > 0), leaky'(c) = (c > 0 ? 1 : 0.1) on the OUTPUT c: with a pinned output of exactly 0 the
    derivative is 0 / 0.1, whatever the pre-activation (ops.act_grad's contract, csrc/train_ops.hip act_grad_kernel)"""
    c, _, _ = _witness(2)
    ref = R.evaluate(c)
    pins = R.pins_of(ref)
    pins["y3"] = torch.zeros_like(pins["y3"])                     # every y3 pinned dead
    pins["y"] = -pins["y"].abs()                                   # every y on the 0.1 branch
    out = R.evaluate(c, pins=pins)
    assert not out["y3"].any() and not out["dw3t"].any() and not out["db3"].any() and not out["dVp"].any()
    zp = torch.where(ref["y"] > 0, ref["y"], ref["y"] / 0.1)       # f_p (pre-activation)
    assert torch.allclose(out["y"], 0.1 * zp, rtol=1e-12, atol=0)


# ---- constants and CSR against the product ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one row", "permuted ladder Q3", "hub Q5", "Q65 N40"])
def test_constants_and_csr_are_the_products(name):
    """the edge list against GossipBatch on the host; C6 / C3 / C2 against gossip_reference.scalars taken the way
    gnn_model.gossip_forward_train takes ops.gossip_scalars: (g0, g1) = (1, 0) gives (deg_lo, s_lo, deg_hi, x) and
    (0, 0) gives (deg_hi, s_hi, deg_hi, x)"""
    import numpy as np
    from desco_amd.batch import GossipBatch
    from desco_amd.graphs import GraphSet
    c = R.trunk_case(name)
    G, N, Q = c["G"], c["N"], c["Q"]
    b = GossipBatch(GraphSet.from_edge_lists([(N, G.edges)]), "cpu", x=c["x"])
    assert np.array_equal(b.rowptr.numpy(), G.rowptr) and torch.equal(b.x, c["x"])
    ne = int(G.rowptr[-1])
    assert np.array_equal(b.col.numpy()[:ne], G.col[:ne]) and len(G.col) == max(ne, 1)
    ones, zeros = torch.ones(Q), torch.zeros(Q)
    sa, _ = GR.scalars(c["x"], G, ones, zeros)
    sb, _ = GR.scalars(c["x"], G, zeros, zeros)
    sa, sb = sa.reshape(N * Q, 4), sb.reshape(N * Q, 4)
    deg_lo, s_lo, deg_hi, xr, s_hi = sa[:, 0], sa[:, 1], sa[:, 2], sa[:, 3], sb[:, 1]
    one = torch.ones_like(xr)
    C6, C3, C2 = R.constants(G, c["x"])
    assert torch.equal(C6, torch.stack([deg_hi, deg_lo - deg_hi, s_hi, s_lo - s_hi, xr, one], 1))
    assert torch.equal(C3, torch.stack([deg_hi, deg_lo - deg_hi, one], 1)) and torch.equal(C2, torch.stack([xr, one], 1))
    assert torch.equal(C6.float(), c["C6"]) and torch.equal(C3.float(), c["C3"]) and torch.equal(C2.float(), c["C2"])
    assert torch.equal(sb[:, 0], deg_hi) and int(deg_lo.sum()) == int(deg_hi.sum()) == Q * ne // 2


# ---- reachability of the GPU gate -------------------------------------------------------------------------------------
def _all_cases():
    out = []
    for name, _, _, _, seed, drops in R.TRUNK_CASES:
        out += [(f"{name}, drop {d}", (lambda n=name: R.trunk_case(n)), d, seed) for d in (None,) + tuple(drops)]
    for name, _, seed, drops in R.DEEP_CASES:
        out += [(f"{name}, drop {d}", (lambda n=name: R.deep_case(n)), d, seed) for d in (None,) + tuple(drops)]
    return out


def _exact_in_any_order(c, k):
    """tensors without a rounding: no term at all (mag == 0: a node without neighbours), or sums of one term that is
    an operand itself.  There E_f32 == 0 and the gate asks the kernels for the exact value too."""
    if c["R"] == 1:
        return k.startswith("hh") or k.startswith("dg") or k == "db7"
    return False


@pytest.mark.parametrize("name,make,drop,seed", _all_cases(), ids=[n for n, _, _, _ in _all_cases()])
def test_a_second_fp32_summation_order_meets_the_gate(name, make, drop, seed):
    c = make()
    if drop is not None:
        c["factors"] = R.bernoulli_factors(c, drop, 900 + seed)
    L = c["L"]
    ref, m = R.evaluate(c, backward=False), R.mag(c, backward=False)
    f32, chunked = R.evaluate(c, torch.float32, backward=False), R.evaluate(c, torch.float32, chunk=32, backward=False)
    for k in R.ACTIVATIONS(L):
        e1, e2 = R.scaled_error(f32[k], ref[k], m[k])[0], R.scaled_error(chunked[k], ref[k], m[k])[0]
        print(f"[parity] gossip trunk reference {name} {k}: E_f32 {e1:.2e}, E_chunk {e2:.2e}, ratio {e2 / max(e1, 1e-300):.2f} (gate 4)")
        assert torch.isfinite(m[k]).all() and e1 < 1e-5 and e2 <= 4 * e1, k
        assert e1 > 0 or (_exact_in_any_order(c, k) and e2 == 0), k
    # every layer alive (the 9-layer case keeps O(1) activations)
    for l in range(1, L + 1):
        live = ref[f"h{l}"] > 0
        rms = float(ref[f"h{l}"][live].pow(2).mean().sqrt()) if live.any() else 0.0
        assert live.float().mean() > 0.1 and 0.05 < rms < 50, (l, float(live.float().mean()), rms)
    # forward and backward pinned to the masks of the fp32 forward
    pins = R.pins_of(f32)
    ref, m = R.evaluate(c, pins=pins), R.mag(c, pins)
    f32, chunked = R.evaluate(c, torch.float32, pins=pins), R.evaluate(c, torch.float32, pins=pins, chunk=32)
    assert set(ref) == set(R.ACTIVATIONS(L) + R.GRADIENTS(L))
    for k in ref:
        e1, e2 = R.scaled_error(f32[k], ref[k], m[k])[0], R.scaled_error(chunked[k], ref[k], m[k])[0]
        print(f"[parity] gossip trunk reference {name} {k} (pinned): E_f32 {e1:.2e}, E_chunk {e2:.2e}, "
              f"ratio {e2 / max(e1, 1e-300):.2f} (gate 4)")
        assert torch.isfinite(m[k]).all() and e1 < 1e-5 and e2 <= 4 * e1, k
        assert e1 > 0 or (_exact_in_any_order(c, k) and e2 == 0), k
    # the bounds are not trivially true, and the regimes hold what they promise
    if c["R"] > 1:
        for k in R.GRADIENTS(L):
            assert (m[k] > 0).float().mean() > 0.5, k
    iso = torch.from_numpy(c["G"].deg == 0)
    if L > 1 and iso.any():
        assert (m["hh1"].view(c["N"], c["Q"], H)[iso] == 0).all()
    if c["regime"] == "x1e6":
        for t in (ref, m):
            assert not t["dV0"][R.ZERO_Q, 2:5].any() and not t["dVp"][R.ZERO_Q, 0].any()
        assert (ref["dV0"][R.ZERO_Q, :2] != 0).float().mean() > 0.5 and float(c["x"].max()) > 9e5
    if c["regime"] == "deadrelu":
        D = R.DEAD_COLS
        for t in (ref, m):
            for k, v in (("db3", t["db3"][D]), ("dw3t", t["dw3t"][:, D]), ("db5", t["db5"][D]), ("dw5t", t["dw5t"][:, D]),
                         ("dw7", t["dw7"][D]), ("dV0", t["dV0"][:, :, D]), ("dwtp", t["dwtp"][D]), ("dwt1", t["dwt1"][H:][D])):
                assert not v.any(), k
        assert not ref["h1"][:, D].any() and not ref["y3"][:, D].any() and not ref["y5"][:, D].any()
    if c["regime"] == "g1exact":
        assert (c["g"][0] == 0).any() and (c["g"][0] == 1).any()


# ---- the gate catches chain errors ------------------------------------------------------------------------------------
def _touched(mut, L):
    layer = lambda l: [f"dV{l}", f"dwt{l}", f"dg{l}"]                                 # noqa: E731
    if mut == "gate_t":          # dh_l wrong for l <= L - 1: layer 0, and the layers l <= L - 2 that read dh_{l+1}
        return ["dV0"] + [k for l in range(1, L - 1) for k in layer(l)]
    if mut == "wtp_swap":        # dh_1 and dh_2 wrong: layer 0 and layer 1
        return ["dV0"] + layer(1)
    if mut == "sites_swap":      # dzp and dz_1 wrong: everything below post_mp.3
        return ["dV0", "dwtp", "dVp"] + [k for l in range(1, L) for k in layer(l)]
    if mut == "p_swap":          # other factors in the forward too: everything but db7 = sum dpred
        return [k for k in R.ACTIVATIONS(L) + R.GRADIENTS(L) if k != "db7"]
    if mut == "dg_sign":
        return [f"dg{l}" for l in range(1, L)]
    if mut == "wt_shift":        # layer 2 read with layer 1's weights: dg_2, dh_2 and everything below it
        return ["dg2", "dV0"] + layer(1)
    raise KeyError(mut)


_MUT_CASES = [(f"ladder Q29, drop {d}", (lambda: R.trunk_case("ladder Q29")), d, True) for d in R.DROPS] + \
             [(f"deep L3, drop {d}", (lambda: R.deep_case("deep L3")), d, True) for d in R.DROPS] + \
             [("ladder Q29 signed weights, drop (0.3, 0.1)", (lambda: R.trunk_case("ladder Q29 signed weights")), R.DROPS[0], False),
              ("deep L3 signed weights, drop (0.0, 0.3)", (lambda: R.deep_case("deep L3 signed weights")), R.DROPS[1], False)]


@pytest.mark.parametrize("name,make,drop,ceiling", _MUT_CASES, ids=[c[0] for c in _MUT_CASES])
def test_the_gate_catches_chain_errors(name, make, drop, ceiling):
    """g_l where 1 - g_l belongs in the transposed gather; the first two 64-row blocks of wtp swapped in the dh
    products; the factors of sites H2 and POST swapped in the backward only; p_layer and p_post swapped; the hi part of
    the dg term with the wrong sign; layer 1's wt read for layer 2 in the backward (L = 3).  Each in fp64 in the
    reference itself.  On the dropout and L = 3 cases (aligned weights) each is above the 1e-4 ceiling of the GPU gate
    on every tensor it touches, and above 4 E_f32, the other half of the gate.  On their twins with zero-mean weights
    the terms of a gradient cancel to 1e-4 .. 1e-8 of ``mag``, so that a chain error of the gradient's own size lies
    BELOW the ceiling there (measured: 4e-8 .. 2e-3, printed); those cases rely on the 4 E_f32 half alone, which each
    error exceeds by orders of magnitude."""
    c = make()
    L = c["L"]
    c["factors"] = R.bernoulli_factors(c, drop, 77)
    ref, m = R.evaluate(c), R.mag(c)
    f32 = R.evaluate(c, torch.float32, pins=R.pins_of(ref))
    muts = [mu for mu in R.MUTATIONS if mu != "wt_shift" or L >= 3] + ["p_swap"]
    for mu in muts:
        if mu == "p_swap":
            bad = R.evaluate(dict(c, factors=R.bernoulli_factors(c, drop, 77, swap_p=True)))
        else:
            bad = R.evaluate(c, mutate=mu)
        touched = _touched(mu, L)
        for k in ref:
            e = R.scaled_error(bad[k], ref[k], m[k])[0]
            if k in touched:
                ef = R.scaled_error(f32[k], ref[k], m[k])[0]
                print(f"[mutation] {name}: {mu} on {k}: scaled error {e:.2e} = {e / CEILING:.2g} x the ceiling {CEILING:.0e}, "
                      f"{e / (4 * ef):.2g} x 4 E_f32")
                assert e > 4 * ef and (e > CEILING or not ceiling), (mu, k, e, ef)
            elif mu != "p_swap":
                assert e == 0, (mu, k, e)                          # and nothing else moves


# ---- the two families whose factor is not 4 ---------------------------------------------------------------------------
def test_the_column_sums_pass_the_factor_4_by_fp32_order_alone():
    """dg_l and db3 are a few values, each ONE sum over every node / row.  The reduction orders of the kernels that
    form them -- P row groups, each a running sum in row order, folded in order: P = 16 in the bias row of
    linear_bwd_w, P = 4 in colsum_partial_kernel (csrc/train_ops.hip) -- evaluated in float32 HERE, no kernel involved,
    pass 4 x E_f32 of the whole float32 evaluation on the cases of R.CHAIN_EVIDENCE.  R.FACTOR of those families is this
    measurement rounded up to an integer, and 4 for every other tensor."""
    import math
    worst = {"dg": 0.0, "db3": 0.0}
    for kind, name in R.CHAIN_EVIDENCE:
        c = R.deep_case(name) if kind == "deep" else R.trunk_case(name)
        pins = R.pins_of(R.evaluate(c, torch.float32, backward=False))
        ref, m, f32 = R.evaluate(c, pins=pins), R.mag(c, pins), R.evaluate(c, torch.float32, pins=pins)
        for P in (4, 16):
            ch = R.evaluate(c, torch.float32, pins=pins, chains=P)
            for k in ["db3"] + [f"dg{l}" for l in range(1, c["L"])]:
                e1, e2 = R.scaled_error(f32[k], ref[k], m[k])[0], R.scaled_error(ch[k], ref[k], m[k])[0]
                print(f"[parity] gossip trunk reference {name} {k}, {P} row groups in fp32: E_f32 {e1:.2e}, E_chains {e2:.2e}, "
                      f"ratio {e2 / e1:.2f} (gate 4)")
                assert e2 < 1e-6                                   # still an fp32 sum, not an error
                worst[R.family(k)] = max(worst[R.family(k)], e2 / e1)
    for fam, w in worst.items():
        print(f"[parity] gossip trunk reference: worst E_chains / E_f32 of {fam} on the host {w:.2f}; its factor {R.FACTOR[fam]}")
        assert w > 4 and R.FACTOR[fam] == math.ceil(w), (fam, w)
    assert all(R.FACTOR[R.family(k)] == 4 for k in R.ACTIVATIONS(9) + R.GRADIENTS(9) if R.family(k) not in worst)
