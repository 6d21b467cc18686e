"""desco_gossip_fused_f16x3_f32 where an epilogue constant requested ahead has the least time to arrive or crosses a
boundary.  The kernel requests the constants of every epilogue (u, d1, tp, zp_q, b3, b5, w7) inside the weight ring's
in-order LDS stream, one to two pair steps ahead, and waits for them with counted waits (gossip_f16.hip, the comment
above GF16_REQ); zp_q goes through a per-wave LDS row that every query overwrites.  A constant that is read too early or
too late is a wrong or a stale value in one epilogue, so every case here is held

  * per element to the fp64 reference of tests/gossip_reference.py at the gate of tests/test_gossip_kernels_gpu.py
    (E_kernel <= GATE * E_f32, E_f32 measured in the same test), and
  * to bit-identical results over 20 repeated launches (a timing-dependent value differs between launches).

Graphs: isolated nodes only (no neighbour step: the part of a query in front of the GEMM chain is as short as it gets)
with N = 1, 16, 17, 129; `hub` (rows beyond the 15 staged columns); `ladder`.  Q = 1 (every query is a work unit's
first), 5 (one full unit), 6 (a unit of five and a unit of one), 29; with and without the tile order.

Under load: a 64-node graph (isolated nodes, a path, a small hub with more neighbours than staged columns) replicated
until the work units outnumber the device's wave slots 3 : 1 (the sizing of _ticket_copies), Q = 29: every replica's rows
equal the first replica's bit for bit, and the first replica is within the gate of the fp64 reference of the single
graph.

Every test prints one ``[parity]`` line with its worst error / bound."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import gossip_reference as R  # noqa: E402
from test_gossip_kernels_gpu import DEV, GATE, ROW_CAP, Case, _graph  # noqa: E402
from test_train_kernels_gpu import _bitequal  # noqa: E402

from desco_amd import ops  # noqa: E402

REPEATS = 20


def _on_device(G):
    G.rowptr_dev = torch.from_numpy(G.rowptr).to(DEV)
    G.col_dev = torch.from_numpy(G.col).to(DEV)
    G.tile_perm = ops.gossip_tile_order(G.rowptr_dev, G.n)
    return G


def _unit_edges():
    """64 ids: 20 isolated, a path of 24, a star of 1 + 19 (the centre has more neighbours than the 15 staged columns)"""
    path = [(20 + i, 21 + i) for i in range(23)]
    star = [(44, 45 + i) for i in range(19)]
    return 64, path + star


@functools.lru_cache(maxsize=None)
def _const_graph(name):
    if name.startswith("iso"):
        return _on_device(R.Graph(int(name[3:]), []))
    if name == "unit64":
        return _on_device(R.Graph(*_unit_edges()))
    return _graph(name)


class ConstCase(Case):
    """a Case of tests/test_gossip_kernels_gpu.py on one of this file's graphs"""

    def __init__(self, graph, Q, regime, seed):
        self.name = f"{graph} Q={Q} {regime}"
        self.G, self.Q, self.regime = _const_graph(graph), Q, regime
        assert self.G.n * Q <= ROW_CAP
        self.P = R.operands(Q, regime, seed)
        self.x = R.features(self.G.n, Q, regime, seed)
        self.scal4 = R.scalars(self.x, self.G, self.P["g0"], self.P["g1"])[0].float()
        d = {k: v.to(DEV) for k, v in self.P.items() if isinstance(v, torch.Tensor)}
        self.v = {k: d[k] for k in ("g1", "p", "z", "zp", "r", "t", "u", "tp", "d1", "b3", "b5", "w7")}
        self.v["b7"] = self.P["b7"]
        self.v["wstream"], self.v["winv"] = ops.gossip_f16_stream(*[ops.split_f16_planes(d[k])
                                                                    for k in ("w1", "wp", "w3", "w5")])
        self.scal_dev = self.scal4.to(DEV)


@functools.lru_cache(maxsize=2)
def _case(graph, Q, seed):
    return ConstCase(graph, Q, "o1", seed)


GRAPHS = ["iso1", "iso16", "iso17", "iso129", "hub", "ladder"]
QS = [1, 5, 6, 29]
PARAMS = [(g, q, 300 + 10 * i + j, t) for i, g in enumerate(GRAPHS) for j, q in enumerate(QS) for t in (False, True)]


def _gate(c, got, what):
    ref, D, e32 = c.reference()
    assert got.shape == ref.shape and torch.isfinite(got).all(), c.name
    e, i = R.scaled_error(got, ref, D)
    ratio = e / e32 if e32 > 0 else (0.0 if e == 0 else float("inf"))
    node, q = divmod(i, c.Q)
    print(f"[parity] gossip const-ahead {what} {c.name} ({c.G.n} nodes): E_kernel {e:.3e}, E_f32 {e32:.3e}, worst error / "
          f"bound = {ratio / GATE:.3e} (ratio {ratio:.2f}, gate {GATE:.0f})")
    assert ratio <= GATE, (f"{c.name}: E_kernel {e:.3e} > {GATE:.0f} x E_f32 {e32:.3e} at node {node} query {q} (unit "
                           f"{q // 5}, query {q % 5} of its unit): got {float(got.flatten()[i])!r}, ref "
                           f"{float(ref.flatten()[i])!r}")


@pytest.mark.parametrize("graph,Q,seed,tiled", PARAMS,
                         ids=[f"{g}-Q{q}-{'tiled' if t else 'plain'}" for g, q, _, t in PARAMS])
def test_constants_requested_ahead_arrive(graph, Q, seed, tiled):
    c = _case(graph, Q, seed)
    first = c.launch("f16x3", tiled)
    _gate(c, first.cpu(), "tile order" if tiled else "node order")
    for k in range(1, REPEATS):
        again = c.launch("f16x3", tiled)
        assert torch.equal(again, first), f"{c.name}: launch {k} of {REPEATS} differs from the first in " \
                                          f"{int((again != first).sum())} of {first.numel()} elements"


@pytest.mark.parametrize("tiled", [False, True])
def test_replicas_agree_when_every_wave_slot_is_busy(tiled):
    Q = 29
    c = _case("unit64", Q, 400)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    copies = -(-16 * -(-3 * 8 * cus // 6) // 64)                  # units = ceil(N / 16) * 6 >= 3 * 8 * CUs
    n = 64 * copies
    assert -(-n // 16) * 6 >= 3 * 8 * cus and n * Q <= ROW_CAP, (n, cus)
    big = _on_device(R.Graph(*R.concat([_unit_edges()] * copies)))
    scal = c.scal_dev.repeat(copies, 1, 1)
    got = c.launch("f16x3", tiled, G=big, scal=scal)
    assert got.shape == (n, Q)
    rep = got.view(copies, 64, Q)
    differ = (rep != rep[:1]).flatten(1).any(1)
    assert not differ.any(), (f"{int(differ.sum())} of {copies} replicas differ from the first, e.g. replica "
                              f"{int(differ.nonzero()[0])}: {int((rep != rep[:1]).sum())} elements")
    _bitequal(f"gossip const-ahead {copies} replicas of 64 nodes on {cus} CUs, {'tile' if tiled else 'node'} order: "
              f"last replica vs first", rep[-1].contiguous(), rep[0].contiguous())
    _gate(c, rep[0].cpu(), f"first of {copies} replicas, {'tile' if tiled else 'node'} order,")

