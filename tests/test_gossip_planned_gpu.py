"""desco_gossip_planned_f16x3_f32 against desco_gossip_fused_f16x3_f32, bit for bit (torch.equal): the planned kernel reads
its work units' addressing from the per-batch plan, loads through buffer descriptors and takes packed operands, and no value
of the network changes.

Graphs: the first N ids, N = 1, 15, 16, 17, 128, 129, 300, of a 300-node set -- a path (degrees <= 2) on ids 0..99, isolated
ids 100..109, a star whose centre (150) has 40 leaves on both sides of its id (beyond the four neighbour rows of a plan record
and the fifteen of its mask), a ring with chords (degrees 4 to 6) on 200..259, a path on 260..299 -- so N = 128 / 129 end on
whole / ragged groups and tiles; the star alone (41 nodes); `mutag_shaped(24)`; five isolated nodes with an empty `col`.
Q = 1, 4, 5, 6, 29 (units of five queries), with and without the tile order.  Then: two launches in a row, the plan of the
device against the host twin's, and through the pipeline: GOSSIP_PLAN on and off with equal counts and the expected launches, one captured replay equal to eager, and
the routing of batches above the bound and of batches of long rows to the unplanned entry."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gossip_reference as R  # noqa: E402
from helpers import make_models, standard_queries  # noqa: E402

from desco_amd import gnn_model as GM  # noqa: E402
from desco_amd import ops, synthetic  # noqa: E402
from desco_amd.batch import GossipBatch  # noqa: E402
from desco_amd.pipeline import InferencePipeline  # noqa: E402

DEV = "cuda"


def mixed_edges():
    path = [(i, i + 1) for i in range(99)]
    star = [(150, v) for v in list(range(110, 130)) + list(range(160, 180))]
    ring = [(200 + i, 200 + (i + 1) % 60) for i in range(60)] + [(200 + i, 200 + (i + 7) % 60) for i in range(60)] + \
           [(200 + i, 200 + (i + 30) % 60) for i in range(0, 30, 2)]
    tail = [(260 + i, 261 + i) for i in range(39)]
    return 300, path + star + ring + tail


class DevGraph:
    def __init__(self, n, rowptr, col):
        self.n = n
        self.rowptr = rowptr.to(DEV).int().contiguous()
        self.col = col.to(DEV).int().contiguous()
        self.tile_perm = ops.gossip_tile_order(self.rowptr, n)
        self.plans = {t: ops.gossip_plan(self.rowptr, self.col, n, self.tile_perm if t else None) for t in (False, True)}


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "mutag24":
        b = GossipBatch(synthetic.mutag_shaped(24), DEV)
        return DevGraph(b.num_nodes, b.rowptr, b.col)
    if name == "star41":
        G = R.Graph(41, [(20, v) for v in range(41) if v != 20])
    else:
        G = R.Graph(*R.prefix(int(name[1:]), mixed_edges()[1]))
    return DevGraph(G.n, torch.from_numpy(G.rowptr), torch.from_numpy(G.col))


def test_the_graphs_have_the_shapes_they_are_meant_to_have():
    full = R.Graph(*mixed_edges())
    assert full.deg[:100].max() == 2 and (full.deg[100:110] == 0).all() and full.deg[150] == 40
    assert set(full.deg[200:260].tolist()) <= {4, 5, 6} and {4, 5} <= set(full.deg[200:260].tolist())
    nb = full.col[full.rowptr[150]:full.rowptr[151]]
    assert (nb < 150).sum() == 20 and (nb > 150).sum() == 20
    assert R.Graph(*R.prefix(1, mixed_edges()[1])).deg.tolist() == [0]
    assert R.Graph(41, [(20, v) for v in range(41) if v != 20]).deg[20] == 40
    assert graph("mutag24").n > 300


@functools.lru_cache(maxsize=None)
def operands(Q, seed=11):
    P = R.operands(Q, "o1", seed)
    d = {k: v.to(DEV) for k, v in P.items() if isinstance(v, torch.Tensor)}
    v = {k: d[k] for k in ("g1", "p", "z", "zp", "r", "t", "u", "tp", "d1", "b3", "b5", "w7")}
    v["b7"] = P["b7"]
    v["wstream"], v["winv"] = ops.gossip_f16_stream(*[ops.split_f16_planes(d[k]) for k in ("w1", "wp", "w3", "w5")])
    vp = {"g1": v["g1"], "wstream": v["wstream"], "b7": v["b7"],
          "pzz": torch.cat([v["p"], v["z"], v["zp"]], 1).contiguous(),
          "cst": torch.cat([v[k] for k in ("u", "d1", "tp", "b3", "b5", "w7", "r", "t", "winv")]).contiguous()}
    return d["g0"], v, vp


@functools.lru_cache(maxsize=None)
def case(name, Q):
    """(scal4 [N * Q, 4] on the device, the unplanned entry's result in node order): computed once per (graph, Q)"""
    G = graph(name)
    g0, v, _ = operands(Q)
    x = R.features(G.n, Q, "o1", 7 + Q).to(DEV)
    scal = ops.gossip_scalars(x, G.rowptr, G.col, g0, v["g1"]).reshape(-1, 4)
    ref = ops.gossip_fused_f16(scal, G.rowptr, G.col, G.n, Q, v, torch.zeros(2, dtype=torch.int64, device=DEV))
    assert torch.isfinite(ref).all() and float((ref - x).abs().max()) > 0
    return scal, ref


def planned(name, Q, tiled, out=None, queue=None):
    G = graph(name)
    scal, _ = case(name, Q)
    queue = torch.zeros(2, dtype=torch.int64, device=DEV) if queue is None else queue
    got = ops.gossip_planned_f16(scal, G.col, G.n, Q, operands(Q)[2], queue, G.plans[tiled], tiled, out=out)
    assert int(queue.abs().sum()) == 0, "the kernel must leave its queue words zero"
    return got


NAMES = ["n1", "n15", "n16", "n17", "n128", "n129", "n300", "star41", "mutag24"]
QS = [1, 4, 5, 6, 29]


@pytest.mark.parametrize("tiled", [False, True], ids=["plain", "tiled"])
@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("name", NAMES)
def test_planned_entry_changes_no_bit(name, Q, tiled):
    G = graph(name)
    _, ref = case(name, Q)
    got = planned(name, Q, tiled)
    assert got.shape == (G.n, Q)
    bad = (got != ref) | ~torch.isfinite(got)
    assert not bad.any(), (f"{name} Q={Q} tiled={tiled}: {int(bad.sum())} of {ref.numel()} elements differ, first at (node, "
                           f"query) {bad.nonzero()[0].tolist()}")
    if tiled:       # the unplanned entry with the tile order is the same again (its own invariant, kept in view here)
        v = operands(Q)[1]
        again = ops.gossip_fused_f16(case(name, Q)[0], G.rowptr, G.col, G.n, Q, v,
                                     torch.zeros(2, dtype=torch.int64, device=DEV), tile_perm=G.tile_perm)
        assert torch.equal(again, ref)


@pytest.mark.parametrize("name", ["n300", "mutag24"])
def test_two_launches_in_a_row_and_an_out_destination(name):
    Q = 29
    queue = torch.zeros(2, dtype=torch.int64, device=DEV)
    first = planned(name, Q, True, queue=queue)
    out = torch.full_like(first, float("nan"))
    second = planned(name, Q, True, out=out, queue=queue)
    assert second.data_ptr() == out.data_ptr() and torch.equal(first, second) and torch.equal(first, case(name, Q)[1])


@pytest.mark.parametrize("tiled", [False, True], ids=["plain", "tiled"])
@pytest.mark.parametrize("name", ["n129", "n300", "star41"])
def test_device_plan_equals_the_host_twin(name, tiled):
    G = graph(name)
    host = ops.gossip_plan(G.rowptr.cpu(), G.col.cpu(), G.n, G.tile_perm.cpu() if tiled else None)
    assert torch.equal(G.plans[tiled].cpu(), host)
    groups = host.numel() // (16 * ops.GOSSIP_PLAN_REC + 1)
    deg = np.diff(G.rowptr.cpu().numpy())
    assert int(host[groups * 16 * ops.GOSSIP_PLAN_REC:].max()) == deg.max()


@pytest.mark.parametrize("tiled", [False, True], ids=["plain", "tiled"])
def test_batch_without_an_edge_and_an_empty_col(tiled):
    """five isolated nodes with a col tensor of no element (a null pointer): neither the plan builder nor the planned
    entry may ask for it -- rows of degree 0 never read it"""
    n, Q = 5, 6
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    col = torch.zeros(0, dtype=torch.int32, device=DEV)
    g0, v, vp = operands(Q)
    x = R.features(n, Q, "o1", 3).to(DEV)
    scal = ops.gossip_scalars(x, rowptr, col, g0, v["g1"]).reshape(-1, 4)
    tperm = ops.gossip_tile_order(rowptr, n) if tiled else None
    q = torch.zeros(2, dtype=torch.int64, device=DEV)
    ref = ops.gossip_fused_f16(scal, rowptr, col, n, Q, v, q, tile_perm=tperm)
    plan = ops.gossip_plan(rowptr, col, n, tperm)
    assert torch.equal(plan.cpu(), ops.gossip_plan(rowptr.cpu(), col.cpu(), n, None if tperm is None else tperm.cpu()))
    got = ops.gossip_planned_f16(scal, col, n, Q, vp, q, plan, tiled)
    assert torch.isfinite(got).all() and torch.equal(got, ref) and int(q.abs().sum()) == 0


def test_wrapper_refuses_a_plan_of_another_batch_or_order():
    scal, _ = case("n129", 5)
    G = graph("n129")
    q = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="plan was not built"):
        ops.gossip_planned_f16(scal, G.col, G.n, 5, operands(5)[2], q, G.plans[False], True)
    with pytest.raises(ValueError, match="plan was not built"):
        ops.gossip_planned_f16(scal, G.col, G.n, 5, operands(5)[2], q, graph("n300").plans[True], True)


# ---- through the models ---------------------------------------------------------------------------------------------
KEYS = ("node_count", "graph_gossip_count")


def _pipeline_run(monkeypatch, on, capture=False):
    calls = {"planned": 0, "fused": 0}
    real_p, real_f = ops.gossip_planned_f16, ops.gossip_fused_f16

    def count_p(*a, **k):
        calls["planned"] += 1
        return real_p(*a, **k)

    def count_f(*a, **k):
        calls["fused"] += 1
        return real_f(*a, **k)

    monkeypatch.setattr(ops, "gossip_planned_f16", count_p)
    monkeypatch.setattr(ops, "gossip_fused_f16", count_f)
    monkeypatch.setattr(GM, "GOSSIP_PLAN", on)
    nm, gm = make_models(seed=0)
    qids, _ = standard_queries()
    nm, gm = nm.to(DEV), gm.to(DEV)
    nm.set_queries(qids)
    pipe = InferencePipeline(nm, gm, synthetic.mutag_shaped(24), depth=4, device=DEV)
    res = {k: v.clone() for k, v in pipe.run().items() if k in KEYS}
    torch.cuda.synchronize()
    eager_calls = dict(calls)
    rep = None
    if capture:
        pipe.capture()
        rep = {k: v.clone() for k, v in pipe.run_graph().items() if k in KEYS}
        torch.cuda.synchronize()
    return res, eager_calls, len(pipe.gossip_batches), rep


def test_switch_on_and_off_through_the_inference_path(monkeypatch):
    on, calls_on, batches, rep = _pipeline_run(monkeypatch, True, capture=True)
    off, calls_off, batches_off, _ = _pipeline_run(monkeypatch, False)
    assert batches == batches_off >= 1
    assert calls_on == {"planned": batches, "fused": 0}, calls_on
    assert calls_off == {"planned": 0, "fused": batches}, calls_off
    for k in KEYS:
        assert torch.isfinite(on[k]).all() and torch.equal(on[k], off[k]), k
        assert torch.equal(rep[k], on[k]), f"captured replay differs from eager in {k}"


def test_batches_of_long_rows_take_the_unplanned_entry(monkeypatch):
    """a set in which more than 1 / 16 of the nodes has more than four neighbours (wheels) keeps the launches from before
    the switch, and no plan is built for it; the molecule set beside it takes the planned kernel"""
    from desco_amd.graphs import GraphSet
    wheel = (12, [(0, v) for v in range(1, 12)] + [(v, v % 11 + 1) for v in range(1, 12)] +
             [(v, (v + 1) % 11 + 1) for v in range(1, 12)])                       # hub of degree 11, rim nodes of degree 5
    dense = GraphSet.from_edge_lists([wheel] * 6)
    assert GossipBatch(dense, DEV).long_row_share == 1.0
    assert GossipBatch(synthetic.mutag_shaped(24), DEV).long_row_share == 0.0
    calls = {"planned": 0, "fused": 0}
    real_p, real_f = ops.gossip_planned_f16, ops.gossip_fused_f16
    monkeypatch.setattr(ops, "gossip_planned_f16", lambda *a, **k: (calls.__setitem__("planned", calls["planned"] + 1),
                                                                     real_p(*a, **k))[1])
    monkeypatch.setattr(ops, "gossip_fused_f16", lambda *a, **k: (calls.__setitem__("fused", calls["fused"] + 1),
                                                                   real_f(*a, **k))[1])
    nm, gm = make_models(seed=0)
    qids, _ = standard_queries()
    nm, gm = nm.to(DEV), gm.to(DEV)
    nm.set_queries(qids)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(GM, "GOSSIP_PLAN", on)
        pipe = InferencePipeline(nm, gm, dense, depth=4, device=DEV)
        res[on] = {k: v.clone() for k, v in pipe.run().items() if k in KEYS}
        torch.cuda.synchronize()
        assert all(not b._plans for _, _, b in pipe.gossip_batches)
    assert calls["planned"] == 0 and calls["fused"] >= 2
    for k in KEYS:
        assert torch.isfinite(res[True][k]).all() and torch.equal(res[True][k], res[False][k]), k


def test_blocks_above_the_bound_take_the_unplanned_entry(monkeypatch):
    """the routing's bound, with the bound moved down to the test's size instead of a batch of 2^28 rows"""
    monkeypatch.setattr(ops, "gossip_plan_fits", lambda n, q, tiled=True: False)
    on, calls, batches, _ = _pipeline_run(monkeypatch, True)
    assert calls == {"planned": 0, "fused": batches}
    monkeypatch.undo()
    ref, _, _, _ = _pipeline_run(monkeypatch, False)
    for k in KEYS:
        assert torch.equal(on[k], ref[k]), k
