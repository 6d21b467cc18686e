"""The gossip plan (desco_gossip_plan; here its host twin desco_gossip_plan_host, the same routine per node slot) against
its definition written in numpy, and the argument checks of the plan builder and the planned entry point.  CPU only."""
import numpy as np
import pytest
import torch

from desco_amd import _lib, ops

REC = 8


def hand_made():
    """150 nodes (a ragged last group and a ragged second tile) with degrees 0, 1, 4, 5, 15, 16 and 40; every hub sits
    in the middle of its neighbours' ids, so the smaller-id masks are mixed.  Returns (rowptr, col) int32, cols ascending."""
    n = 150
    adj = [set() for _ in range(n)]

    def link(a, b):
        adj[a].add(b)
        adj[b].add(a)

    for leaf in list(range(50, 70)) + list(range(71, 91)):     # node 70: 40 neighbours, 20 smaller and 20 larger
        link(70, leaf)
    for leaf in list(range(0, 8)) + list(range(100, 108)):      # node 20: 16 neighbours
        link(20, leaf)
    for leaf in list(range(8, 15)) + list(range(108, 116)):     # node 30: 15 neighbours
        link(30, leaf)
    for leaf in (15, 16, 120, 121, 122):                        # node 40: 5 neighbours
        link(40, leaf)
    for leaf in (17, 18, 123, 149):                             # node 45: 4 neighbours (one in the last group)
        link(45, leaf)
    deg = np.array([len(a) for a in adj])
    assert {0, 1, 4, 5, 15, 16, 40} <= set(deg.tolist())
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = np.array([j for a in adj for j in sorted(a)], np.int32)
    return rowptr, col


def _deal_tile():
    """slot of every sorted rank of a 128-row tile, built the way desco_gossip_tile_order is defined (desco_hip.h): the
    rows sorted by degree are paired, and the 64 pairs are dealt to the eight waves in snake order -- 0..7, 7..0, 0..7,
    ... -- each wave filling its 16 slots pair by pair."""
    slot_of_rank, filled = {}, [0] * 8
    for pair in range(64):
        rnd, pos = divmod(pair, 8)
        wave = pos if rnd % 2 == 0 else 7 - pos
        for half in (0, 1):
            slot_of_rank[2 * pair + half] = 16 * wave + 2 * filled[wave] + half
        filled[wave] += 1
    assert sorted(slot_of_rank.values()) == list(range(128))
    return slot_of_rank


SLOT_OF_RANK = _deal_tile()


def slot_row(gr, s, tperm):
    """the row of slot s of group gr: in node order rows 16 gr .. 16 gr + 15; with a tile order group gr of a tile
    takes its sorted ranks 16 (gr % 8) .. + 15, rank by rank"""
    if tperm is None:
        return gr * 16 + s
    t0 = (gr >> 3) * 128
    return t0 + int(tperm[t0 + SLOT_OF_RANK[16 * (gr & 7) + s]])


def plan_numpy(rowptr, col, n, tperm):
    groups = (n + 127) // 128 * 8 if tperm is not None else (n + 15) // 16
    plan = np.zeros(groups * (16 * REC + 1), np.int64)
    for gr in range(groups):
        mx = 0
        for s in range(16):
            raw = slot_row(gr, s, tperm)
            valid = raw < n
            row = raw if valid else n - 1
            e0 = int(rowptr[row])
            deg = int(rowptr[row + 1]) - e0 if valid else 0
            nb = col[e0:e0 + deg]
            lt = sum(1 << i for i in range(min(deg, 15)) if nb[i] < row) | (0 if valid else 1 << 31)
            first = [int(nb[i]) if i < deg else row for i in range(4)]
            plan[(gr * 16 + s) * REC:(gr * 16 + s + 1) * REC] = [row, deg, lt] + first + [e0]
            mx = max(mx, deg)
        plan[groups * 16 * REC + gr] = mx
    return (plan & 0xffffffff).astype(np.uint32).view(np.int32)


@pytest.mark.parametrize("tiled", [False, True])
def test_plan_matches_its_definition(tiled):
    rowptr, col = hand_made()
    n = len(rowptr) - 1
    tperm = None
    if tiled:       # any permutation of a tile's 128 rows is a tile order as far as the plan is concerned
        rng = np.random.default_rng(5)
        tperm = np.concatenate([rng.permutation(128) for _ in range((n + 127) // 128)]).astype(np.uint8)
    got = ops.gossip_plan(torch.from_numpy(rowptr), torch.from_numpy(col), n,
                          None if tperm is None else torch.from_numpy(tperm)).numpy()
    ref = plan_numpy(rowptr, col, n, tperm)
    assert got.shape == ref.shape == (_lib.lib().desco_gossip_plan_words(n, int(tiled)),)
    assert np.array_equal(got, ref)
    groups = (len(ref)) // (16 * REC + 1)
    rec = got[:groups * 16 * REC].reshape(groups, 16, REC)
    # every node appears in exactly one live slot; the empty slots take the last row with degree 0
    live = rec[:, :, 2] >= 0
    assert sorted(rec[:, :, 0][live].tolist()) == list(range(n))
    assert (~live).sum() == groups * 16 - n and (rec[:, :, 0][~live] == n - 1).all() and (rec[:, :, 1][~live] == 0).all()
    assert np.array_equal(got[groups * 16 * REC:], rec[:, :, 1].max(1))
    assert 40 in got[groups * 16 * REC:]


def test_plan_of_one_node_and_of_nothing():
    rowptr = torch.zeros(2, dtype=torch.int32)
    col = torch.zeros(1, dtype=torch.int32)
    got = ops.gossip_plan(rowptr, col, 1).numpy()
    assert got.shape == (16 * REC + 1,)
    assert got[:REC].tolist() == [0] * REC and got[16 * REC] == 0
    assert (got[REC:16 * REC].reshape(15, REC)[:, 2] < 0).all()           # fifteen empty slots
    assert ops.gossip_plan(rowptr, col, 0).numel() == 0
    # a batch without an edge may come with an empty col (a null pointer): rows of degree 0 never read it
    iso = ops.gossip_plan(torch.zeros(4, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), 3).numpy()
    assert iso[:3 * REC].reshape(3, REC).tolist() == [[r, 0, 0, r, r, r, r, 0] for r in range(3)] and iso[16 * REC] == 0


def test_plan_builder_and_planned_entry_check_their_arguments():
    L = _lib.lib()
    buf = np.zeros(4096, np.int32)
    p = buf.ctypes.data
    assert p % 16 == 0
    assert L.desco_gossip_plan_words(-1, 0) == -1
    assert L.desco_gossip_plan_words(129, 0) == 9 * (16 * REC + 1) and L.desco_gossip_plan_words(129, 1) == 16 * (16 * REC + 1)
    assert L.desco_gossip_plan_host(None, p, 5, None, p) == -1 and b"desco_gossip_plan_host" in L.desco_last_error()
    assert L.desco_gossip_plan_host(p, p, -1, None, p) == -1
    assert L.desco_gossip_plan_host(None, None, 0, None, None) == 0        # nothing to do
    assert L.desco_gossip_plan(None, p, 5, None, p, None) == -1 and b"desco_gossip_plan" in L.desco_last_error()
    assert L.desco_gossip_plan(p, p, 5, None, p + 4, None) == -1           # a misaligned plan
    assert L.desco_gossip_plan(None, None, 0, None, None, None) == 0

    def planned(scal=p, n=8, q=4, pzz=p, cst=p, plan=p, out=p, queue=p):
        return L.desco_gossip_planned_f16x3_f32(scal, p, n, q, p, pzz, cst, p, 0.0, out, plan, 0, queue, None)

    name = b"desco_gossip_planned_f16x3_f32"
    for bad in (dict(scal=None), dict(plan=None), dict(queue=None), dict(q=0), dict(q=65536), dict(n=-1),
                dict(scal=p + 4), dict(pzz=p + 4), dict(cst=p + 8), dict(plan=p + 4), dict(queue=p + 4), dict(out=p + 2)):
        assert planned(**bad) == -1 and name in L.desco_last_error(), bad
        L.desco_rng_next(None, None, None)                                 # (another message in between)
    assert planned(n=0) == 0
    # the 32-bit bound: num_nodes * num_q * 16 < 2^32, refused on the host before any launch
    assert planned(n=2 ** 28 // 29 + 1, q=29) == -1
    assert name in L.desco_last_error() and b"2^32" in L.desco_last_error()
    assert planned(n=2 ** 28, q=1) == -1 and b"2^32" in L.desco_last_error()
    assert ops.gossip_plan_fits(2 ** 28 // 29, 29) and not ops.gossip_plan_fits(2 ** 28 // 29 + 1, 29)
    assert not ops.gossip_plan_fits(2 ** 28, 1) and ops.gossip_plan_fits(48_000_000 // 29, 29)
    # a plan of 2^32 bytes or more is refused too (Q = 1: 528 bytes of plan per 16 nodes)
    assert not ops.gossip_plan_fits(2 ** 27 + 2 ** 26, 1, tiled=False)


def test_ops_wrappers_refuse_mismatched_operands():
    rowptr, col = hand_made()
    with pytest.raises(ValueError, match="tile_perm is shorter"):
        ops.gossip_plan(torch.from_numpy(rowptr), torch.from_numpy(col), 150, torch.zeros(128, dtype=torch.uint8))
    with pytest.raises(ValueError, match="rowptr is shorter"):
        ops.gossip_plan(torch.from_numpy(rowptr), torch.from_numpy(col), 151)
    with pytest.raises(ValueError, match="host operands"):
        ops.gossip_plan(torch.from_numpy(rowptr).long(), torch.from_numpy(col), 150)


def test_routing_statistic_of_a_batch():
    """GossipBatch.long_row_share, what gnn_model.gossip_takes_plan routes by: the share of nodes beyond four neighbours"""
    from desco_amd import gnn_model as GM
    from desco_amd.batch import GossipBatch
    from desco_amd.graphs import GraphSet
    star6 = (7, [(0, v) for v in range(1, 7)])                    # one node of degree 6 among seven
    path = (9, [(v, v + 1) for v in range(8)])
    assert GossipBatch(GraphSet.from_edge_lists([star6, path]), "cpu").long_row_share == 1 / 16
    assert GossipBatch(GraphSet.from_edge_lists([path]), "cpu").long_row_share == 0.0
    assert GossipBatch(GraphSet.from_edge_lists([star6]), "cpu").long_row_share == 1 / 7
    assert GM.GOSSIP_PLAN_LONG_ROW_SHARE == 1 / 16
