"""desco_pool_post_rows_bf16x6_f32 (ops.pool_post(..., anch_row=idx)): post_mp.0 on the pooled embeddings with the anchor rows
read from a TABLE of their distinct values through one id per neighborhood.  The launch is desco_pool_post_bf16x6_f32 with
another row address, so it must equal that launch on the gathered rows bit for bit (torch.equal): neighborhoods of 1 .. 33
count rows in every alignment to the 16-row tiles, one block, the block boundary and several blocks, tables of one and of
seven rows, constant, permuted and repeated ids, models of 2, 5 and 8 layers."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from desco_amd import ops  # noqa: E402

DEV = "cuda"
H = 64
M = (1, 127, 128, 129, 300)


def _segments(m, seed):
    """m neighborhoods of 1 .. 33 count rows: every length in turn from a seed-dependent start, so that the segments begin at
    every offset of a 16-row tile and span one, two and three tiles"""
    lens = torch.tensor([1 + (7 * seed + 5 * i) % 33 for i in range(m)], dtype=torch.int64)
    seg = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)]).to(torch.int32).to(DEV)
    bits, slot, totals = ops.pool_index_dev(seg, m, int(seg[-1]))
    return seg, bits, slot, int(totals[0])


def _ids(kind, m, U, g):
    if kind == "constant":
        return torch.full((m,), U - 1, dtype=torch.int32)
    if kind == "permutation":                     # every table row in a shuffled order, as often as it takes to fill m ids
        return torch.cat([torch.randperm(U, generator=g) for _ in range((m + U - 1) // U)])[:m].to(torch.int32)
    return torch.randint(0, U, (m,), generator=g).to(torch.int32)       # repeats


@pytest.fixture(scope="module")
def cases():
    """per (m, L): segments, partial arrays and weights, made once and left unchanged"""
    out = {}
    for m in M:
        for L in (2, 5, 8):
            g = torch.Generator().manual_seed(1000 * m + L)
            seg, bits, slot, ns = _segments(m, m + L)
            r = lambda *s: torch.rand(*s, generator=g).to(DEV)              # noqa: E731
            out[m, L] = dict(seg=seg, bits=bits, slot=slot, parts=[r(ns, H) - 0.5 for _ in range(L)], x0=r(H) - 0.5,
                             w0=ops.split_bf16_planes((r(H, H * (L + 1)) - 0.5) * 0.2), b0=r(H) - 0.5,
                             tab=r(7, H * (L + 1)) - 0.5, g=g)
    return out


@pytest.mark.parametrize("L", [2, 5, 8])
@pytest.mark.parametrize("m", M)
def test_rows_through_ids_equal_the_gathered_rows(cases, m, L):
    c = cases[m, L]
    post = lambda anch, **kw: ops.pool_post(anch, c["parts"], c["bits"], c["slot"], c["seg"], c["x0"], c["w0"], c["b0"],   # noqa: E731
                                            ops.ACT_LEAKY, 0.1, **kw)
    lens = (c["seg"][1:] - c["seg"][:-1]).tolist()
    assert len(lens) == m and 1 <= min(lens) and max(lens) <= 33 and (m < 33 or set(lens) == set(range(1, 34)))
    for U in (1, 7):
        tab = c["tab"][:U].contiguous()
        for kind in ("constant", "permutation", "repeats"):
            idx = _ids(kind, m, U, c["g"]).to(DEV)
            want = post(tab[idx.long()].contiguous())
            got = post(tab, anch_row=idx)
            assert got.shape == (m, H) and torch.isfinite(got).all() and torch.equal(got, want), (U, kind)
            # a table inside a wider tensor (row stride above its width), as a column slice of the anchor output would be
            wide = torch.zeros(U, H * (L + 1) + 64, device=DEV)
            wide[:, :H * (L + 1)] = tab
            assert torch.equal(post(wide[:, :H * (L + 1)], anch_row=idx), want), (U, kind, "stride")
    # the result depends on the table row: two different rows give different outputs (the ids are not ignored)
    if m > 1:
        a, b = post(c["tab"], anch_row=torch.zeros(m, dtype=torch.int32, device=DEV)), \
            post(c["tab"], anch_row=torch.ones(m, dtype=torch.int32, device=DEV))
        assert not torch.equal(a, b)


@pytest.mark.parametrize("m,L", [(129, 8), (300, 5), (1, 2)])
def test_no_ids_is_the_old_call(cases, m, L):
    c = cases[m, L]
    g = torch.Generator().manual_seed(m)
    anch = (torch.rand(m, H * (L + 1), generator=g) - 0.5).to(DEV)
    args = (anch, c["parts"], c["bits"], c["slot"], c["seg"], c["x0"], c["w0"], c["b0"], ops.ACT_LEAKY, 0.1)
    old = ops.pool_post(*args)
    assert torch.equal(ops.pool_post(*args, anch_row=None), old)
    assert torch.equal(ops.pool_post(*args, anch_row=torch.arange(m, dtype=torch.int32, device=DEV)), old)
    # ... and the old entry point itself, which forwards without ids
    from desco_amd import _lib
    import ctypes
    out = torch.empty(m, H, device=DEV)
    pa = (ctypes.c_void_p * L)(*[p.data_ptr() for p in c["parts"]])
    rc = _lib.lib().desco_pool_post_bf16x6_f32(anch.data_ptr(), anch.stride(0), L, c["w0"].data_ptr(), 64, c["b0"].data_ptr(),
                                               ops.ACT_LEAKY, 0.1, out.data_ptr(), 64, m, c["seg"].data_ptr(),
                                               c["bits"].data_ptr(), c["slot"].data_ptr(), pa, c["x0"].data_ptr(), 16,
                                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(out, old)
