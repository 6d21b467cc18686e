"""gnn_model.ANCHOR_POST_FUSED: the anchor MLP, the pooled sums and post_mp.0 in one launch
(desco_anchor_pool_post_f16x3_f32) against the two launches it replaces (desco_gemm_f16x3_f32 writing the anchor rows,
desco_pool_post_bf16x6_f32 reading them): same values in the same order, so h0 and the logits are bit-identical."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from desco_amd import ops  # noqa: E402
from desco_amd.batch import NeighborhoodBatch  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402
from desco_amd.partition import build_partition  # noqa: E402

from helpers import golden_graphs, make_models, random_family_graphs, standard_queries  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def setup():
    nm, _ = make_models(seed=0)
    nm = nm.to(DEV)
    nm.set_queries(standard_queries()[0])
    stars = [(k + 1, [(0, v) for v in range(1, k + 1)]) for k in (1, 2, 15, 16, 17, 31, 32, 33)]     # count rows up to 33
    graphs = golden_graphs(max_n=60) + random_family_graphs(11, 30) + stars
    part = build_partition(GraphSet.from_edge_lists(graphs), 4)
    ok = np.diff(part.count_ptr) <= 33
    runs, a = [], None
    for i in range(part.num_neigh + 1):
        if i < part.num_neigh and ok[i] and a is None:
            a = i
        if (i == part.num_neigh or not ok[i]) and a is not None:
            runs.append((a, i))
            a = None
    a, b = max(runs, key=lambda r: r[1] - r[0])
    return nm, part, a, b


def _run(nm, batch, fused):
    import desco_amd.gnn_model as GM
    GM.ANCHOR_POST_FUSED = fused
    try:
        with torch.no_grad():
            h0 = GM._shmp_pooled(nm.emb_model, batch, fuse_post0=True)
            assert isinstance(h0, GM._PostMp0)
            return h0.h0.clone(), nm._logits(batch, exp2=False).clone()
    finally:
        GM.ANCHOR_POST_FUSED = True


def test_fused_anchor_post_changes_no_bit(setup):
    nm, part, a, b = setup
    # the longest eligible run, a prefix shorter than one 128-row tile, and one that is not a multiple of 128
    for lo, hi in ((a, b), (a, min(b, a + 77)), (a, min(b, a + 128 + 77)), (a + 5, min(b, a + 5 + 300))):
        batch = NeighborhoodBatch(part.slice(lo, hi), DEV)
        assert batch.max_count_rows() <= 33
        h_on, y_on = _run(nm, batch, True)
        h_off, y_off = _run(nm, batch, False)
        print(f"[anchor post] {batch.num_graphs} neighborhoods, max |dh0| = {float((h_on - h_off).abs().max()):.3e}")
        assert torch.isfinite(y_on).all()
        assert torch.equal(h_on, h_off)
        assert torch.equal(y_on, y_off)


def test_fused_anchor_post_repeats(setup):
    nm, part, a, b = setup
    batch = NeighborhoodBatch(part.slice(a, b), DEV)
    ref, _ = _run(nm, batch, True)
    for _ in range(3):
        assert torch.equal(_run(nm, batch, True)[0], ref)


def test_fused_anchor_post_captured_replay_equals_eager():
    """InferencePipeline.capture(): the pass with the one-launch anchor + post_mp.0 replays bit for bit (graphs of at
    most 12 nodes: no neighborhood has more than 33 count rows, so every batch takes the fused launch)."""
    import desco_amd.gnn_model as GM
    from desco_amd.pipeline import InferencePipeline
    assert GM.ANCHOR_POST_FUSED
    nm, gm = make_models(seed=0)
    nm, gm = nm.to(DEV), gm.to(DEV)
    nm.set_queries(standard_queries()[0])
    gs = GraphSet.from_edge_lists(golden_graphs(max_n=12))
    pipe = InferencePipeline(nm, gm, gs, depth=4, device=DEV)
    eager = {k: v.clone() for k, v in pipe.run().items()}
    pipe.capture()
    rep = pipe.run_graph()
    torch.cuda.synchronize()
    for k in ("neigh_count", "node_count", "graph_gossip_count"):
        assert torch.equal(eager[k], rep[k]), k


def test_anchor_post_direct_call_with_an_empty_segment(setup):
    """A segment without count rows (seg_ptr[b] == seg_ptr[b + 1], here one past the last tile) adds no partial rows:
    its pooled row is the anchor row alone (block 0: plus 0 * x0).  Checked against an fp64 reference."""
    torch.manual_seed(3)
    nm, part, a, b = setup
    batch = NeighborhoodBatch(part.slice(a, min(b, a + 200)), DEV)
    pbits, pslot, nslots = batch.pool_index()
    L, H = 8, 64
    B = batch.num_graphs + 1
    seg = torch.cat([batch.count_ptr, batch.count_ptr[-1:]])
    canon = torch.rand(B, 9 * H, device=DEV)
    wa, ba = torch.randn(9 * H, 8 * H, device=DEV) * 0.05, torch.randn(9 * H, device=DEV) * 0.1
    w0, b0 = torch.randn(H, 9 * H, device=DEV) * 0.05, torch.randn(H, device=DEV) * 0.1
    x0 = torch.rand(H, device=DEV)
    parts = [torch.rand(nslots, H, device=DEV) for _ in range(L)]
    bound = canon[:, H:].abs().amax(dim=1).contiguous()
    got = ops.anchor_pool_post(canon[:, H:], ops.split_f16_planes(wa), ba, bound, parts, pbits, pslot, seg, x0,
                               ops.split_bf16_planes(w0), b0, ops.ACT_LEAKY, 0.1)
    # the two launches it replaces, on the same arguments
    anch = ops.gemm_f16x3(canon[:, H:], ops.split_f16_planes(wa), ba, act=ops.ACT_LEAKY, slope=0.1, row_scale=bound)
    two = ops.pool_post(anch, parts, pbits, pslot, seg, x0, ops.split_bf16_planes(w0), b0, ops.ACT_LEAKY, 0.1)
    assert torch.equal(got[:-1], two[:-1])
    # the empty segment's row in fp64
    lk = torch.nn.functional.leaky_relu
    an = lk(canon[-1:, H:].double() @ wa.double().T + ba.double(), 0.1)
    ref = lk(an @ w0.double().T + b0.double(), 0.1)
    err = float((got[-1:].double() - ref).abs().max() / (1 + ref.abs().max()))
    print(f"[anchor post] empty segment: rel err {err:.2e}")
    assert err < 1e-5
