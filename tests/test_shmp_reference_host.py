"""tests/shmp_reference.py on the host, before any GPU is involved:
  * the reference against a dense-matrix evaluation of the same contract (one 0/1 matrix per relation slot, a 0/1
    pooling matrix, no ``index_add_``) on 12 rows and 2 layers, forward and every gradient, so that it is not its own
    only witness; the dense form with two slot matrices exchanged, and with one layer's pool seed dropped, must differ;
  * the gate of tests/test_shmp_trunk_kernels_gpu.py (E_kernel <= 4 E_f32 on the scale ``mag``) is reachable by a
    correct fp32 implementation: a second fp32 summation order (K in 32-wide chunks, summed from the last chunk) stays
    within 4x the whole-K fp32 evaluation's error on every case that file runs, forward and backward, both pinned to the
    relu masks of the fp32 forward;
  * the bounds are not trivially true: mag > 0 on every live element, and exactly 0 on the dead columns."""
import numpy as np
import pytest
import torch

import shmp_reference as R

H = R.H


def _kept(case):
    """the elements of xall a dropout factor does not zero (all of them without dropout)"""
    if case["factors"] is None:
        return ...
    return torch.stack(case["factors"]) != 0


# ---- dense witness ----------------------------------------------------------------------------------------------------
def _dense(case, S, Pm, swap=False, drop_seed=None):
    """The contract with matrices: S[s] [N, N] 0/1 (row i, slot s gathers row j), Pm [B, Nc] 0/1.  ``swap``: slot
    matrices 0 and 1 exchanged; ``drop_seed``: the pooling of that layer's rows carries no gradient."""
    d = lambda t: t.double().clone().requires_grad_()                                 # noqa: E731
    x0, Wt, bias = d(case["x0"]), [d(w) for w in case["Wt"]], [d(b) for b in case["bias"]]
    anchor = None if case["anchor"] is None else tuple(d(t) for t in case["anchor"])
    if swap:
        S = [S[1], S[0]] + list(S[2:])
    B, Nc = Pm.shape
    X = [x0]
    for l in range(Wt[0].shape[0]):
        rows = []
        for g, (r0, r1, su) in enumerate(case["groups"]):
            A = torch.cat([(S[s] @ X[-1])[r0:r1] for s in range(su)] + [X[-1][r0:r1]], 1)
            rows.append(torch.relu(A @ Wt[g][l] + bias[g][l]))
        x = torch.cat(rows)
        X.append(x if case["factors"] is None else x * case["factors"][l].double())
    pooled = torch.cat([Pm @ (x.detach() if l == drop_seed else x)[:Nc] for l, x in enumerate(X)], 1)
    if anchor is not None:
        a = torch.cat([x[Nc:] for x in X], 1) @ anchor[0] + anchor[1]
        pooled = pooled + torch.where(a > 0, a, 0.1 * a)
    pooled.backward(case["dpooled"].double())
    out = {"xall": torch.stack(X[1:]).detach(), "pooled": pooled.detach(), "dx0": x0.grad}
    for g in range(len(Wt)):
        out[f"dwt{g}"], out[f"dbias{g}"] = Wt[g].grad, bias[g].grad
    if anchor is not None:
        out["daw"], out["dab"] = anchor[0].grad, anchor[1].grad
    return out


def _query_witness():
    """two graphs, 7 + 5 rows, triangle and other edges on the same rows, unequal slot degrees; dropout factors"""
    graphs = [(7, [(0, 1), (1, 2), (0, 2), (2, 3), (3, 4), (4, 5), (3, 5), (5, 6)]), (5, [(0, 1), (1, 2), (2, 3), (1, 3)])]
    N = 12
    case = R.query_case(graphs, 2, "o1", 3, factors=R.bernoulli_factors(N, 2, 0.2, 4))
    A = torch.zeros(N, N, dtype=torch.float64)
    off = 0
    for n, edges in graphs:
        for a, b in edges:
            A[off + a, off + b] = A[off + b, off + a] = 1
        off += n
    tri = A * ((A @ A) > 0)                                                           # the edge's ends share a neighbour
    Pm = torch.zeros(2, N, dtype=torch.float64)
    Pm[0, :7], Pm[1, 7:] = 1, 1
    return case, [tri, A - tri], Pm


def _anchor_witness():
    """10 count rows (4 slots) + 2 canonical rows (2 slots), random 0/1 slot matrices; the CSR is read off them"""
    g = torch.Generator().manual_seed(11)
    Nc, B, N = 10, 2, 12
    S = [(torch.rand(N, N, generator=g) < 0.25).double() for _ in range(4)]
    for s in (2, 3):
        S[s][Nc:] = 0                                                                 # canonical rows: slots 0 and 1
    cnt = torch.stack([S[s].sum(1) for s in range(4)], 1).reshape(-1).long()           # virtual row 4 i + s
    vrowptr = torch.cat([torch.zeros(1, dtype=torch.long), cnt.cumsum(0)])
    vcol = torch.cat([S[s][i].nonzero().flatten() for i in range(N) for s in range(4)])
    count_ptr = np.array([0, 4, 10])
    case = R.neighborhood_case(vrowptr, vcol, count_ptr, N, 2, 12)
    Pm = torch.zeros(B, Nc, dtype=torch.float64)
    Pm[0, :4], Pm[1, 4:] = 1, 1
    return case, S, Pm


@pytest.mark.parametrize("witness", [_query_witness, _anchor_witness])
def test_reference_equals_the_dense_matrix_formula(witness):
    case, S, Pm = witness()
    assert case["x0"].shape[0] == 12 and case["Wt"][0].shape[0] == 2
    got, m, want = R.evaluate(case), R.mag(case), _dense(case, S, Pm)
    assert set(want) <= set(got)
    for k in want:
        e, _ = R.scaled_error(got[k], want[k], m[k])
        print(f"[parity] trunk reference vs dense-matrix formula, {witness.__name__} {k}: max |d| / mag = {e:.2e}")
        assert (m[k] > 0)[_kept(case) if k == "xall" else ...].float().mean() > 0.9 and e <= 1e-13, k
    # known wrong forms must show at this size
    sw = _dense(case, S, Pm, swap=True)
    assert (sw["pooled"] - want["pooled"]).abs().max() > 1e-3 and (sw["dx0"] - want["dx0"]).abs().max() > 1e-3
    for l in range(3):
        ds = _dense(case, S, Pm, drop_seed=l)
        assert (ds["dx0"] - want["dx0"]).abs().max() > 1e-3, l
        if l > 0:
            assert max((ds[k] - want[k]).abs().max() for k in want if k.startswith("dwt")) > 1e-3, l


def test_reference_csr_is_the_products_query_csr():
    """query_csr (written from the contract) against desco_amd.batch.QueryBatch on the host, on every shape"""
    from desco_amd.batch import QueryBatch
    graphs = list(R.SHAPES) + [R.wheel(20), R.star(9), R.random_graph(30, 1)]
    qb = QueryBatch(graphs, "cpu")
    vrowptr, vcol, seg_ptr = R.query_csr(graphs)
    assert torch.equal(qb.vrowptr.long(), vrowptr) and torch.equal(qb.vcol.long(), vcol)
    assert torch.equal(qb.graph_ptr.long(), seg_ptr)
    deg = (vrowptr[1:] - vrowptr[:-1]).view(-1, 2)
    assert deg[:, 0].max() >= 19 and deg[:, 1].max() >= 8          # a hub in either slot


# ---- reachability of the GPU gate -------------------------------------------------------------------------------------
def _neighborhood(L, seed, p=None):
    from helpers import golden_graphs
    from desco_amd.graphs import GraphSet
    from desco_amd.partition import build_partition
    part = build_partition(GraphSet.from_edge_lists(golden_graphs(max_n=41)[:10]), 4)
    fac = None if p is None else R.bernoulli_factors(part.num_rows, L, p, seed)
    return R.neighborhood_case(part.vrowptr, part.vcol, part.count_ptr, part.num_rows, L, seed, fac)


def _standard_queries(L, seed):
    from helpers import standard_queries
    return R.query_case(standard_queries()[1], L, "o1", seed)


def _all_cases():
    out = [(f"small / {n}", (lambda g=g, L=L, r=r, i=i: R.query_case(g, L, r, 100 + i)))
           for i, (n, g, L, r, _) in enumerate(R.SMALL_CASES)]
    out += [(f"graphs / {n}", (lambda g=g, L=L, r=r, i=i: R.query_case(g, L, r, 200 + i)))
            for i, (n, g, L, r, _) in enumerate(R.GRAPH_CASES)]
    out += [(f"graphs / {n}", (lambda g=g, L=L, p=p, i=i: R.query_case(
        g, L, "o1", 300 + i, R.bernoulli_factors(sum(k for k, _ in g), L, p, 300 + i))))
        for i, (n, g, L, p, _) in enumerate(R.DROP_CASES)]
    out += [("node / neighborhood", lambda: _neighborhood(8, 400)),
            ("node / neighborhood dropout", lambda: _neighborhood(8, 401, 0.2)),
            ("node / standard queries L8", lambda: _standard_queries(8, 402)),
            ("node / standard queries L1", lambda: _standard_queries(1, 403))]
    return out


@pytest.mark.parametrize("name,make", _all_cases(), ids=[n for n, _ in _all_cases()])
def test_a_second_fp32_summation_order_meets_the_gate(name, make):
    case = make()
    # forward, unpinned (relu is continuous: no mask to agree on)
    ref, m = R.evaluate(case, backward=False), R.mag(case, backward=False)
    f32, chunked = R.evaluate(case, torch.float32, backward=False), R.evaluate(case, torch.float32, 32, backward=False)
    for k in ("xall", "pooled"):
        live = m[k] > 0
        if "dead relu" in name:                            # zero weights and bias: no term at all
            live.view(*live.shape[:-1], -1, H)[..., 1 if k == "pooled" else 0:, R.ZERO_COLS] = True
        if k == "pooled" and case["factors"] is not None:
            live = live[:, :H]                             # (a one-row graph's later blocks are 0 where its row is dropped)
        assert torch.isfinite(m[k]).all() and live[_kept(case) if k == "xall" else ...].all(), k
        e1, e2 = R.scaled_error(f32[k], ref[k], m[k])[0], R.scaled_error(chunked[k], ref[k], m[k])[0]
        print(f"[parity] trunk reference {name} {k}: E_f32 {e1:.2e}, E_chunk {e2:.2e}, ratio {e2 / max(e1, 1e-300):.2f} (gate 4)")
        assert 0 < e1 < 1e-5 and e2 <= 4 * e1, k
    # forward and backward pinned to the masks of the fp32 forward
    pins = R.pins_of(f32["xall"])
    apin = (f32["anch"] > 0).double() if "anch" in f32 else None
    ref, m = R.evaluate(case, pins=pins, anchor_pin=apin), R.mag(case, pins, apin)
    f32 = R.evaluate(case, torch.float32, pins=pins, anchor_pin=apin)
    chunked = R.evaluate(case, torch.float32, 32, pins=pins, anchor_pin=apin)
    for k in ref:
        e1, e2 = R.scaled_error(f32[k], ref[k], m[k])[0], R.scaled_error(chunked[k], ref[k], m[k])[0]
        print(f"[parity] trunk reference {name} {k} (pinned): E_f32 {e1:.2e}, E_chunk {e2:.2e}, ratio {e2 / max(e1, 1e-300):.2f} (gate 4)")
        assert 0 < e1 < 1e-5 and e2 <= 4 * e1, k
        # the bound is not trivially true: mag > 0 wherever a term exists, exactly 0 where the case leaves none
        if k == "xall":                                    # live exactly where the pinned mask and the factor are
            live = torch.stack(pins) > 0
            if case["factors"] is not None:
                live &= torch.stack(case["factors"]) != 0
            assert torch.equal(m[k] > 0, live), k
        elif k == "pooled":
            assert (m[k][:, :H] > 0).all(), k              # (a later block is 0 where every row of the graph is masked)
        elif k in ("dx0", "dab", "anch"):
            assert (m[k] > 0).all(), k
        elif k == "daw":
            assert (m[k][:H] > 0).all(), k                 # (the rows that meet x0; a later row may be masked everywhere)
        else:                                              # dbias / dwt of group g: live where a row of the group is
            r0, r1, _ = case["groups"][int(k[-1])]
            col_live = live[:, r0:r1].any(1)                                         # [L, 64]
            if k.startswith("dbias"):
                assert torch.equal(m[k] > 0, col_live), k
            else:                                          # layer 0, self block: x0 has no zero
                assert torch.equal(m[k][0, -H:] > 0, col_live[0].expand(H, H)), k
                assert (m[k][:, :, ~col_live.any(0)] == 0).all(), k
            if "dead relu" in name:                        # exactly 0 on the dead columns, in mag and in the reference
                for cols in (R.DEAD_COLS, R.ZERO_COLS):
                    assert (m[k][..., cols] == 0).all() and (ref[k][..., cols] == 0).all(), k
                    assert not col_live[:, cols].any() and (ref["xall"][..., cols] == 0).all()
                assert col_live.float().mean() > 0.5


def test_dropout_factors_matter_and_scale():
    """the stand-in factors are 0 or 1 / (1 - p), and a case with them differs from the case without"""
    name, graphs, L, p, _ = R.DROP_CASES[1]
    N = sum(n for n, _ in graphs)
    fac = R.bernoulli_factors(N, L, p, 1)
    s = float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32))
    assert all(set(f.unique().tolist()) == {0.0, s} for f in fac)
    a = R.evaluate(R.query_case(graphs, L, "o1", 1, fac), backward=False)["pooled"]
    b = R.evaluate(R.query_case(graphs, L, "o1", 1), backward=False)["pooled"]
    assert ((a - b).abs() / (1 + b.abs())).max() > 1e-3
