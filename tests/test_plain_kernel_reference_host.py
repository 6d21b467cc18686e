"""The host reference of the fused plain-layer kernel (tests/plain_kernel_reference.py) checked on the CPU without trusting
itself: the formula against a dense adjacency-matrix form in float64, and the GPU test's gate proven reachable on every
case -- the kernel's documented arithmetic restated on the host (row scales, fp16 hi / lo split, three products per
32-wide K step, the second split of relu(h)) stays within 4x the float32 evaluation's error and gives relu(b2) bit for
bit on the rows whose relu(h) is all zero."""
import numpy as np
import pytest
import torch

import plain_kernel_reference as P
import wide_reference as W


def emulate(case):
    """the kernel's arithmetic on the host -> [N, Wp] float32 (the sum inside one 32-wide step is numpy's, not the MFMA's)"""
    f32 = np.float32
    z = W.gather((case["x"], case["rowptr"], case["col"]), torch.float32).numpy()
    if case["s"]:
        z = z + (f32(case["s"]) * case["x"].numpy()).astype(f32)

    def product(v, Wt, bias):
        Wt = Wt.numpy().astype(f32)
        ws = W._pow2_scale(np.abs(Wt).max().astype(f32))
        wh, wl = W._split(Wt * ws)
        sc = W._pow2_scale(np.abs(v).max(1))
        ah, al = W._split(v * sc[:, None])
        tmp = np.zeros(v.shape, f32)
        for k in range(0, v.shape[1], 32):
            tmp = tmp + al[:, k:k + 32] @ wh[k:k + 32]
            tmp = tmp + ah[:, k:k + 32] @ wl[k:k + 32]
            tmp = tmp + ah[:, k:k + 32] @ wh[k:k + 32]
        return tmp * ((f32(1) / sc) * (f32(1) / ws))[:, None] + bias.numpy().astype(f32)
    h = product(z.astype(f32), case["W1"], case["b1"])
    if case["W2"] is not None:
        h = product(np.maximum(h, f32(0)), case["W2"], case["b2"])
    return torch.from_numpy(np.maximum(h, f32(0)))


def test_formula_equals_the_dense_adjacency_form():
    case = P.make("instantiation Wp 128 mats 2")
    N = case["x"].shape[0]
    A = torch.zeros(N, N, dtype=torch.float64)
    deg = case["rowptr"][1:] - case["rowptr"][:-1]
    A.index_put_((torch.repeat_interleave(torch.arange(N), deg), case["col"]), torch.ones(case["col"].numel(), dtype=torch.float64),
                 accumulate=True)
    x = case["x"].double()
    z = A @ x + 0.25 * x
    want = torch.relu(torch.relu(z @ case["W1"].double() + case["b1"].double()) @ case["W2"].double() + case["b2"].double())
    assert float((P.evaluate(case) - want).abs().max()) <= 1e-11 * float(want.abs().max())
    assert int(deg.max()) >= 301 and set(range(10)) <= set(deg[37:240].tolist())


@pytest.mark.parametrize("name", list(P.CASES))
def test_the_gate_is_reachable_on_every_case(name):
    case = P.make(name)
    r = slice(case["row0"], case["row0"] + case["num_rows"])
    ref, m, f32 = P.evaluate(case)[r], P.mag(case)[r], P.evaluate(case, torch.float32)[r]
    got = emulate(case)[r]
    ek, _ = P.scaled_error(got, ref, m)
    ef, _ = P.scaled_error(f32, ref, m)
    print(f"[parity] emulated kernel, {name}: E {ek:.3e}, E_f32 {ef:.3e}, ratio {ek / ef if ef else 0:.2f}")
    assert ek <= 4 * ef and ek <= 1e-4 and bool((got.double()[m == 0] == 0).all())
    if case["mats"] == 2:
        for i in case["dead"]:
            assert torch.equal(got[i - case["row0"]], torch.relu(case["b2"]))
    else:
        for i in case["bare"]:
            assert torch.equal(got[i - case["row0"]], torch.relu(case["b1"]))
    if case["H"] is not None:
        assert not got[:, case["H"]:].any()
    if case["regime"] == "dead":
        assert len(case["dead"]) == 3 and bool((P.evaluate(case)[r] > 0).any())
