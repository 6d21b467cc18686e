"""tests/gossip_reference.py on the host, before any GPU is involved:
  * the reference against a dense-matrix evaluation of the same contract (adjacency matrices A_lo / A_hi, no
    ``index_add_``) on a 12-node graph, so that it is not its own only witness;
  * the gate of tests/test_gossip_kernels_gpu.py (E_kernel <= 4 E_f32 on the scale D) is reachable by a correct fp32
    implementation: a second fp32 summation order (K in 32-wide chunks, summed from the last chunk) stays within 4x the
    whole-K fp32 evaluation's error on every operand regime."""
import numpy as np
import pytest
import torch

import gossip_reference as R


def _random_graph(n, seed):
    rng = np.random.default_rng(seed)
    e = [(int(rng.integers(v)), v) for v in range(1, n) if rng.random() < 0.85]
    e += [(int(rng.integers(n)), int(rng.integers(n))) for _ in range(2 * n)]
    h = n // 3
    e += [(h, v) for v in range(0, n, 2)]
    return n, e


def test_reference_equals_the_dense_matrix_formula():
    n, Q = 12, 5
    edges = [(0, 1), (0, 5), (1, 2), (1, 11), (2, 3), (3, 4), (3, 9), (4, 5), (5, 6), (5, 7), (5, 8), (5, 9), (5, 10),
             (6, 11), (8, 9), (9, 10)]                                               # id 7's only neighbour is lower
    G = R.Graph(n, edges)
    P = R.operands(Q, "g1exact", 3)
    x = R.features(n, Q, "o1", 3)
    A = torch.zeros(n, n, dtype=torch.float64)
    for a, b in edges:
        A[a, b] = A[b, a] = 1
    A_lo, A_hi = torch.tril(A, -1), torch.triu(A, 1)                                  # [i, j]: j < i / j > i
    d = lambda k: P[k].double()                                                       # noqa: E731
    xd = x.double()
    g0, g1 = d("g0"), d("g1")
    dlo, dhi = A_lo.sum(1, keepdim=True), A_hi.sum(1, keepdim=True)
    a0, a1 = g0 * dlo + (1 - g0) * dhi, g1 * dlo + (1 - g1) * dhi
    b0 = g0 * (A_lo @ xd) + (1 - g0) * (A_hi @ xd)
    scal, _ = R.scalars(x, G, P["g0"], P["g1"])
    want = torch.stack([a0, b0, a1, xd], -1)
    assert (scal - want).abs().max() <= 1e-13 * want.abs().max()
    h1 = torch.relu(a0[..., None] * d("p") + b0[..., None] * d("r") + xd[..., None] * d("t") + d("z"))   # [n, Q, 64]
    hh = g1[None, :, None] * torch.einsum("ij,jqf->iqf", A_lo, h1) + \
        (1 - g1)[None, :, None] * torch.einsum("ij,jqf->iqf", A_hi, h1)
    h2 = torch.relu(torch.cat([hh, h1], -1) @ d("w1").t() + a1[..., None] * d("u") + d("d1"))
    y1 = torch.cat([h1, h2], -1) @ d("wp").t() + xd[..., None] * d("tp") + d("zp")
    y1 = torch.where(y1 > 0, y1, 0.1 * y1)
    y2 = torch.relu(y1 @ d("w3").t() + d("b3"))
    y3 = torch.relu(y2 @ d("w5").t() + d("b5"))
    out = xd + float(torch.tensor(P["b7"], dtype=torch.float32)) + y3 @ d("w7")
    got, D, _ = R.net(want, G, P)
    err = ((got - out).abs() / D).max().item()
    print(f"[parity] gossip reference vs dense-matrix formula: max |d| / D = {err:.2e}")
    assert (D > 0).all() and err <= 1e-13
    # a direction swapped or a gate complemented must show at this size: the dense formula with A_lo / A_hi exchanged
    hh_sw = g1[None, :, None] * torch.einsum("ij,jqf->iqf", A_hi, h1) + \
        (1 - g1)[None, :, None] * torch.einsum("ij,jqf->iqf", A_lo, h1)
    assert (hh_sw - hh).abs().max() > 1e-3


@pytest.mark.parametrize("regime", R.REGIMES)
def test_a_second_fp32_summation_order_meets_the_gate(regime):
    Q = 29
    G = R.Graph(*R.concat([R.ladder_edges(), _random_graph(463, 3)]))
    assert G.n == 700
    P = R.operands(Q, regime, 5)
    x = R.features(G.n, Q, regime, 5)
    scal4 = R.scalars(x, G, P["g0"], P["g1"])[0].float()
    ref, D, stats = R.net(scal4, G, P)
    assert torch.isfinite(D).all() and (D > 0).all()
    whole, _, _ = R.net(scal4, G, P, torch.float32)
    chunked, _, _ = R.net(scal4, G, P, torch.float32, chunk=32)
    e1, _ = R.scaled_error(whole, ref, D)
    e2, _ = R.scaled_error(chunked, ref, D)
    print(f"[parity] gossip reference {regime}: E_f32 (whole K) {e1:.2e}, E_f32 (32-wide chunks, last first) {e2:.2e}, "
          f"ratio {e2 / e1:.2f} (gate 4); zero h1 / h2 rows {stats['h1_zero']:.2f} / {stats['h2_zero']:.2f}")
    assert 0 < e1 < 1e-5 and e2 <= 4 * e1
    if regime == "deadrelu":
        assert 0.05 <= stats["h1_zero"] <= 0.95 and 0.05 <= stats["h2_zero"] <= 0.95
