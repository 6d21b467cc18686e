"""desco_class_rows_pool_f32 alone: the pooled sums of the table layers on representative neighborhoods, bit for bit
(torch.equal) against the walk it replaces -- ops.table_rows_pool over every count row of the block -- with post_mp.0's
((p0 + p1) + p2) formed in torch from the walk's partial rows of the same neighborhoods, and through ops.pool_post itself: the
launch on the representatives' compact segments gives the rows the launch on the whole block gives for them.

The row pointer is hand-built: segments of 1, 2, 15, 16, 17, 32 and 33 rows starting at rows 0, 1 and 15 of a 16-row tile --
one, two and three pieces, a piece of one row, a segment that ends exactly on a tile boundary."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from desco_amd import ops  # noqa: E402

DEV = "cuda"
ROWS, STARTS = (1, 2, 15, 16, 17, 32, 33), (0, 1, 15)


def _count_ptr():
    """(count_ptr, {(n, f): neighborhood}): every n of ROWS at every start f of STARTS; fillers set the alignment"""
    cp, where = [0], {}
    for n in ROWS:
        for f in STARTS:
            gap = (f - cp[-1]) % 16
            if gap:
                cp.append(cp[-1] + gap)
            where[(n, f)] = len(cp) - 1
            cp.append(cp[-1] + n)
    return np.asarray(cp, dtype=np.int64), where


CP, WHERE = _count_ptr()


def _slots(cp, bits, slot, b):
    """the (at most three) slots of segment b, as post_mp.0 finds them"""
    a, e = int(cp[b]), int(cp[b + 1])
    t0, t1, f = a >> 4, (e - 1) >> 4, a & 15
    s = [int(slot[t0]) + bin(int(bits[t0]) & 0xFFFFFFFF & ((1 << f) - 1)).count("1")]
    s += [int(slot[t0 + j]) for j in (1, 2) if t1 >= t0 + j]
    return s


@pytest.fixture(scope="module")
def block():
    """per (L, table rows): tables, ids, the walk's partial rows and the reference sums of every neighborhood (computed once)"""
    assert all(CP[b] & 15 == f and CP[b + 1] - CP[b] == n for (n, f), b in WHERE.items())
    B, nc = len(CP) - 1, int(CP[-1])
    cp = torch.from_numpy(CP.astype(np.int32)).to(DEV)
    bits, slot, totals = ops.pool_index_dev(cp, B, nc)
    nslots = int(totals[0])
    hb, hs = bits.cpu().numpy(), slot.cpu().numpy()
    out = {"cp": cp, "index": (bits, slot, nslots)}
    g = torch.Generator().manual_seed(5)
    for L in (2, 5, 8):
        for nt in (1, 300):
            tables = [torch.randn((nt, 64), generator=g).to(DEV) for _ in range(L)]
            ids = [torch.randint(0, nt, (nc,), generator=g).to(torch.int32).to(DEV) for _ in range(L)]
            parts = [torch.full((nslots, 64), float("nan"), device=DEV) for _ in range(L)]
            pool = (bits, slot, parts[-1])
            for k in range(L - 1):
                pool = pool + (tables[k], ids[k], parts[k])
            ops.table_rows_pool(tables[-1], ids[-1], nc, None, pool)
            assert not any(torch.isnan(p).any() for p in parts)
            ref = torch.zeros((L, B, 64), device=DEV)
            for b in range(B):
                s = _slots(CP, hb, hs, b)
                for k in range(L):
                    p = [parts[k][j] for j in s] + [torch.zeros(64, device=DEV)] * (3 - len(s))
                    ref[k, b] = (p[0] + p[1]) + p[2]
            out[(L, nt)] = (tables, ids, parts, ref)
    return out


def _run(block, L, nt, rep):
    """the kernel on the representatives ``rep``: (its partial arrays [L][nslots_u, 64], rep_ptr, bits, slot, nslots_u)"""
    tables, ids, _, _ = block[(L, nt)]
    rows = np.diff(CP)[rep]
    rep_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)).to(DEV)
    bits, slot, totals = ops.pool_index_dev(rep_ptr, len(rep), int(rows.sum()))
    nslots = int(totals[0])
    parts = [torch.full((nslots, 64), float("nan"), device=DEV) for _ in range(L)]
    ops.class_rows_pool(list(zip(tables, ids, parts)), block["cp"], int(CP[-1]), torch.as_tensor(rep, dtype=torch.int64).to(DEV),
                        rep_ptr, bits, slot, nslots)
    torch.cuda.synchronize()
    return parts, rep_ptr, bits, slot, nslots


REPS = {"all": list(range(len(CP) - 1)),
        "one": [WHERE[(33, 15)]],
        "seven, unordered, the block's last": [len(CP) - 2, WHERE[(16, 0)], WHERE[(1, 15)], WHERE[(17, 15)], WHERE[(32, 1)],
                                                WHERE[(2, 15)], WHERE[(15, 1)]],
        "the same neighborhood twice": [WHERE[(33, 1)], WHERE[(33, 1)], WHERE[(16, 1)]]}


@pytest.mark.parametrize("reps", list(REPS))
@pytest.mark.parametrize("nt", [1, 300])
@pytest.mark.parametrize("L", [2, 5, 8])
def test_first_slot_holds_the_walks_combined_sum_and_the_others_zeros(block, L, nt, reps):
    rep = REPS[reps]
    ref = block[(L, nt)][3]
    parts, rep_ptr, bits, slot, nslots = _run(block, L, nt, rep)
    hp, hb, hs = rep_ptr.cpu().numpy().astype(np.int64), bits.cpu().numpy(), slot.cpu().numpy()
    seen = set()
    for u, b in enumerate(rep):
        s = _slots(hp, hb, hs, u)
        assert not seen & set(s)
        seen |= set(s)
        for k in range(L):
            assert torch.equal(parts[k][s[0]], ref[k, b]), (u, b, k)
            assert all(torch.equal(parts[k][j], torch.zeros(64, device=DEV)) for j in s[1:]), (u, b, k)
    assert seen == set(range(nslots))                                         # every slot written: no NaN left
    assert not any(torch.isnan(p).any() for p in parts)


@pytest.mark.parametrize("L", [2, 5, 8])
def test_post_mp0_on_the_compact_segments_gives_the_blocks_rows(block, L):
    tables, ids, walk_parts, _ = block[(L, 300)]
    B = len(CP) - 1
    g = torch.Generator().manual_seed(L)
    anch = torch.randn((5, 64 * (L + 1)), generator=g).to(DEV)
    arow = torch.randint(0, 5, (B,), generator=g).to(torch.int32).to(DEV)
    w = ops.split_bf16_planes((0.2 * torch.randn((64, 64 * (L + 1)), generator=g)).to(DEV))
    x0, bias = torch.randn(64, generator=g).to(DEV), torch.randn(64, generator=g).to(DEV)
    bits, slot, _ = block["index"]
    full = ops.pool_post(anch, walk_parts, bits, slot, block["cp"], x0, w, bias, ops.ACT_LEAKY, 0.1, anch_row=arow)
    rep = REPS["seven, unordered, the block's last"]
    parts, rep_ptr, ubits, uslot, _ = _run(block, L, 300, rep)
    idx = torch.as_tensor(rep, dtype=torch.int64).to(DEV)
    got = ops.pool_post(anch, parts, ubits, uslot, rep_ptr, x0, w, bias, ops.ACT_LEAKY, 0.1, anch_row=arow[idx].contiguous())
    assert torch.isfinite(full).all() and torch.equal(got, full[idx])


def test_gather_rows():
    g = torch.Generator().manual_seed(1)
    src = torch.randn((37, 29), generator=g).to(DEV)
    rows = torch.randint(0, 37, (1001,), generator=g).to(torch.int32).to(DEV)
    buf = torch.zeros((1003, 29), device=DEV)
    out = ops.gather_rows(src, rows, out=buf[1:1002])
    assert out.data_ptr() == buf[1:1002].data_ptr() and torch.equal(buf[1:1002], src[rows.long()])
    assert not buf[0].any() and not buf[1002].any()
    wide = torch.randn((3, 70), generator=g).to(DEV)
    assert torch.equal(ops.gather_rows(wide, rows[:9] % 3), wide[(rows[:9] % 3).long()])
