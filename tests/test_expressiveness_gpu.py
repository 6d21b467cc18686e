"""Colour refinement on the GPU (csrc/wl_refine_dev.hip): the kernel against the host twin bit for bit -- signatures,
final colours and status -- on every input of the host tests, on segment sizes around the wave and the wave / workgroup
boundaries, on rows long enough for the whole-wave walk, on slices, streams and guarded outputs; the routing above the
device bound; the kernel's own guard; and the colour classes against the model kernels they claim to bound."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import wl_reference as R  # noqa: E402
from helpers import LOGIT_TOL, assert_logits_close, log_space_err, make_models, standard_queries  # noqa: E402
from desco_amd import _lib, expressiveness as X, synthetic  # noqa: E402
from desco_amd.batch import GraphBatch, NeighborhoodBatch  # noqa: E402
from desco_amd.graphs import GraphSet  # noqa: E402
from desco_amd.partition import build_partition  # noqa: E402

DEV = "cuda"
W = X.WAVE_ROWS


def assert_device_equals_host(b, view, rounds, init=None):
    want = X.refine(b, view, rounds, backend="host", init=init, keep_colours=True)
    got = X.refine_device(b, view, rounds, DEV, init=init, keep_colours=True)
    for f, dt in (("signature", torch.int64), ("colours", torch.int64), ("status", torch.int32)):
        x = getattr(got, f)
        assert x.is_cuda and x.dtype == dt, f
    got = got.cpu()
    assert np.array_equal(got.status, want.status) and not want.status.any()
    assert np.array_equal(got.signature, want.signature), (view, rounds)
    assert np.array_equal(got.colours, want.colours), (view, rounds)
    return want


@pytest.mark.parametrize("name", sorted(R.blocks()))
def test_device_equals_host_twin(name):
    b, views = R.blocks()[name]
    for view in views:
        for rounds in (0, 1, 8):
            want = assert_device_equals_host(b, view, rounds)
        assert len(set(want.signature.tolist())) > 1                    # a constant answer must not pass
    res = X.refine(b, views[-1], 8, backend="device")
    assert X.last_backend == res.last_backend == "device" and np.array_equal(res.signature, want.signature)
    auto = X.refine(b, views[-1], 8, backend="auto")
    assert X.last_backend == "device" and np.array_equal(auto.signature, want.signature) and auto.colours is None


def random_block(sizes, anchored, seed, slots=4, degree=3.0):
    """Segments of ``sizes`` rows (anchor included when ``anchored``): random symmetric entries inside every segment, a
    random slot per entry; the count rows of all segments first, then the anchors"""
    rng = np.random.default_rng(seed)
    counts = [s - 1 if anchored else s for s in sizes]
    seg_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    nc, S = int(seg_ptr[-1]), len(sizes)
    num_rows = nc + (S if anchored else 0)
    rows_of = [[] for _ in range(num_rows * slots)]
    for i, s in enumerate(sizes):
        ids = list(range(seg_ptr[i], seg_ptr[i + 1])) + ([nc + i] if anchored else [])
        for _ in range(int(degree * s / 2) if s > 1 else 0):
            a, c = rng.integers(s, size=2)
            if a != c:
                rows_of[ids[a] * slots + int(rng.integers(slots))].append(ids[c])
                rows_of[ids[c] * slots + int(rng.integers(slots))].append(ids[a])
    vrowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows_of])]).astype(np.int32)
    vcol = np.array([c for r in rows_of for c in r], dtype=np.int32)
    return X.Block(vrowptr, vcol, num_rows, slots, seg_ptr, nc if anchored else -1)


SIZES = [1, 2, 63, 64, 65, W - 1, W, W + 1, 3 * W + 5, 1, 257, 40, 1025]


@pytest.mark.parametrize("anchored", [True, False])
def test_segment_sizes_around_the_wave_and_the_workgroup_threshold(anchored):
    b = random_block(SIZES, anchored, seed=5)
    assert X.segment_rows(b).tolist() == SIZES
    rng = np.random.default_rng(11)
    for view in X.VIEWS:
        for rounds in (0, 1, 8):
            assert_device_equals_host(b, view, rounds)
    assert_device_equals_host(b, "shmp", 8, init=rng.integers(-2 ** 63, 2 ** 63 - 1, size=b.num_rows, dtype=np.int64))
    for bound in (W - 1, W, W + 1):          # one launch per form: the wave kernel up to W rows, the workgroup above
        small = random_block([s for s in SIZES if s <= bound], anchored, seed=6)
        want = X.refine(small, "hetero", 8, backend="host", keep_colours=True)
        got = X._device(small, X.view_groups("hetero", 4), 8, None, True, DEV, launch_bound=bound).cpu()
        assert not got.status.any() and np.array_equal(got.signature, want.signature)
        assert np.array_equal(got.colours, want.colours)


def hub_graphs():
    star = lambda n, hub: (n, sorted((min(hub, v), max(hub, v)) for v in range(n) if v != hub))     # noqa: E731
    wheel = (301, star(301, 300)[1] + [(v, (v + 1) % 300) for v in range(299)] + [(0, 299)])   # hub over a 300-cycle: no
    return GraphSet.from_edge_lists([star(301, 300), star(301, 0), (wheel[0], sorted(wheel[1]))])  # clique above K3


def test_long_rows_are_walked_by_the_whole_wave():
    g = hub_graphs()
    for batch, views in ((GraphBatch(g, "cpu"), ("plain", "shmp")), (build_partition(g, 4), X.VIEWS),
                         (build_partition(g, 4, restricted=True), X.VIEWS)):
        b = X._block(batch)
        vr = np.asarray(b.vrowptr.numpy() if isinstance(b.vrowptr, torch.Tensor) else b.vrowptr, dtype=np.int64)
        assert np.diff(vr[::b.slots]).max() >= 300                      # a row far above the whole-wave threshold
        for view in views:
            for rounds in (0, 1, 8):
                assert_device_equals_host(b, view, rounds)


@pytest.fixture(scope="module")
def syn_part():
    """a thinned syn_1827-shaped schedule (40 graphs, 10 to 800 nodes) as neighborhoods"""
    return build_partition(synthetic.syn_1827_shaped(40), 4)


def test_largest_syn_neighborhood_and_mixed_buckets(syn_part):
    rows = np.diff(syn_part.count_ptr) + 1
    assert rows.max() > 4 * W and (rows <= W).any()                     # both kernel forms, several buckets
    big = int(np.argmax(rows))
    idx = np.unique(np.concatenate([np.arange(0, syn_part.num_neigh, max(1, syn_part.num_neigh // 50)), [big]]))
    sub = syn_part.select(idx)
    for view in X.VIEWS:
        for rounds in (0, 1, 8):
            assert_device_equals_host(sub, view, rounds)
    want = X.refine(syn_part, "shmp", 8, backend="host")
    got = X.refine(NeighborhoodBatch(syn_part, DEV), "shmp", 8, backend="auto")          # every bucket in one call
    assert X.last_backend == "device" and np.array_equal(got.signature, want.signature)
    assert np.array_equal(want.signature[idx], X.refine(sub, "shmp", 8, backend="host").signature)
    print(f"[syn] {syn_part.num_neigh} neighborhoods, largest {rows.max()} rows, "
          f"{len(set(want.signature.tolist()))} classes after 8 rounds")


def test_data_set_classes_on_the_device_equal_the_host():
    g = R.graph_sets()["cox2"]
    for restricted, view in ((False, "shmp"), (True, "plain")):
        want = X.neighborhood_classes(g, 4, 8, view, restricted, backend="host")
        dev = X.neighborhood_classes_device(g, 4, 8, view, restricted)
        assert all(getattr(dev, f).is_cuda for f in ("signature", "class_id", "class_size", "neigh_index"))
        got = X.neighborhood_classes(g, 4, 8, view, restricted, backend="auto")
        assert X.last_backend == "device"
        for c in (dev.cpu(), got):
            for f in ("signature", "class_id", "class_size", "neigh_index"):
                assert np.array_equal(getattr(c, f), getattr(want, f)), f
            assert c.num_classes == want.num_classes
    want = X.graph_classes(g, 8, "shmp", backend="host")
    for c in (X.graph_classes_device(g, 8, "shmp").cpu(), X.graph_classes(g, 8, "shmp", backend="device")):
        assert np.array_equal(c.signature, want.signature) and np.array_equal(c.class_id, want.class_id)
    with pytest.raises(ValueError, match="hetero"):
        X.graph_classes_device(g, 8, "hetero")


def test_slices_guard_words_and_another_stream():
    b, _ = R.blocks()["cox2/ball"]
    S = len(b.seg_ptr) - 1
    want = X.refine(b, "shmp", 8, backend="host", keep_colours=True)
    ids = np.arange(1, S, 3)
    part = X.refine_device(b, "shmp", 8, DEV, keep_colours=True, seg_ids=ids, fill=-7).cpu()
    mine = np.zeros(S, dtype=bool)
    mine[ids] = True
    assert np.array_equal(part.signature[mine], want.signature[mine]) and (part.signature[~mine] == -7).all()
    assert (part.status[mine] == 0).all() and (part.status[~mine] == X.NOT_LAUNCHED).all()
    row_mine = np.concatenate([np.repeat(mine, np.diff(b.seg_ptr)), mine])
    assert np.array_equal(part.colours[row_mine], want.colours[row_mine]) and (part.colours[~row_mine] == -7).all()
    # the outputs between sentinel words: nothing is written beside them
    guard = 64
    flat = {"sig": torch.full((S + 2 * guard,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV),
            "col": torch.full((b.num_rows + 2 * guard,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV),
            "st": torch.full((S + 2 * guard,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)}
    out = (flat["sig"][guard:guard + S], flat["col"][guard:guard + b.num_rows], flat["st"][guard:guard + S])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):                                     # ... on a stream that is not the default one
        X._device(b, X.view_groups("shmp", 4), 8, None, True, DEV, out=out)
    stream.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), want.signature) and np.array_equal(out[1].cpu().numpy(), want.colours)
    assert not out[2].cpu().numpy().any()
    for t in flat.values():
        sentinel = 0x5A5A5A5A5A5A5A5A if t.dtype == torch.int64 else 0x5A5A5A5A
        assert (t[:guard] == sentinel).all() and (t[-guard:] == sentinel).all()


def test_segments_above_the_bound_go_to_the_host():
    b = random_block(SIZES, True, seed=9)
    want = X.refine(b, "shmp", 8, backend="host", keep_colours=True)
    with pytest.raises(RuntimeError, match="DESCO_WL_DEV_MAX_ROWS"):
        X.refine(b, "shmp", 8, backend="device", max_rows=300)
    with pytest.raises(RuntimeError, match="DESCO_WL_DEV_MAX_ROWS"):
        X.refine_device(b, "shmp", 8, DEV, max_rows=300)
    merged = X.refine(b, "shmp", 8, backend="auto", max_rows=300, keep_colours=True)
    assert X.last_backend == merged.last_backend == "device+host" and not merged.status.any()
    assert np.array_equal(merged.signature, want.signature) and np.array_equal(merged.colours, want.colours)
    same = X.refine(b, "shmp", 8, backend="auto", max_rows=max(SIZES))
    assert X.last_backend == "device" and np.array_equal(same.signature, want.signature)
    # a segment above the kernel's own limit: refused by the entry point, by name; "auto" merges
    huge = random_block([5, X.DEVICE_MAX_ROWS + 1, 70], True, seed=10, degree=2.0)
    with pytest.raises(RuntimeError, match="desco_wl_refine_dev.*DESCO_WL_DEV_MAX_ROWS"):
        X.refine(huge, "plain", 2, backend="device")
    got = X.refine(huge, "plain", 2, backend="auto")
    assert X.last_backend == "device+host" and not got.status.any()
    assert np.array_equal(got.signature, X.refine(huge, "plain", 2, backend="host").signature)
    at_limit = random_block([X.DEVICE_MAX_ROWS, 3], True, seed=12, degree=2.0)          # the largest that fits
    got = X.refine(at_limit, "shmp", 3, backend="auto")
    assert X.last_backend == "device"
    assert np.array_equal(got.signature, X.refine(at_limit, "shmp", 3, backend="host").signature)


def test_entry_point_refuses_before_any_launch():
    """desco_wl_refine_dev checks its arguments on the host: none of these calls reaches the GPU."""
    L = _lib.lib()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data
    grp = np.arange(4, dtype=np.int32)

    def call(vrowptr=p, slots=4, group=grp.ctypes.data, seg_ptr=p, S=1, rounds=8, ids=None, num_ids=0, max_rows=64,
             sig=p, status=p, init=None):
        return L.desco_wl_refine_dev(vrowptr, p, 8, slots, group, seg_ptr, S, 7, init, rounds, ids, num_ids, max_rows, sig,
                                     None, status, None)

    def rejects(rc, word):
        assert rc == -1
        msg = L.desco_last_error()
        assert b"desco_wl_refine_dev" in msg and word in msg, msg
        assert L.desco_rng_next(None, None, None) == -1          # (resets the message for the next case)

    assert call(S=0) == 0                                         # nothing to do
    rejects(call(rounds=65), b"rounds")
    rejects(call(slots=5), b"slots")
    rejects(call(group=np.array([0, 4, 0, 0], np.int32).ctypes.data), b"group entry")
    rejects(call(group=None), b"group is null")
    rejects(call(S=-1), b"negative")
    rejects(call(max_rows=-1), b"negative max_rows")
    rejects(call(max_rows=X.DEVICE_MAX_ROWS + 1), b"DESCO_WL_DEV_MAX_ROWS")
    rejects(call(vrowptr=None), b"vrowptr is null")
    rejects(call(seg_ptr=None), b"seg_ptr is null")
    rejects(call(sig=None), b"sig is null")
    rejects(call(status=None), b"status is null")
    rejects(call(init=p + 4), b"aligned")


def test_the_kernel_guards_itself():
    """A bad column: the kernel checks every entry before it indexes LDS with one, so the segment gets status -1, nothing
    else of it is written and its neighbours' results are intact.  The same for a segment over the launch's bound."""
    b = random_block([40, 70, 200, 9, 64], True, seed=21)
    want = X.refine(b, "shmp", 8, backend="host", keep_colours=True)
    for where, bad_id in ((1, 0), (2, b.num_rows - 1), (1, -5), (2, 2 ** 31 - 1)):
        vc = b.vcol.copy()
        at = int(b.vrowptr[int(b.seg_ptr[where]) * 4 + 5])              # an entry of the segment's second row
        assert b.seg_ptr[where] <= vc[at] < b.seg_ptr[where + 1] or vc[at] == b.anchor_base + where
        vc[at] = bad_id
        broken = b._replace(vcol=vc)
        host = X.refine(broken, "shmp", 8, backend="host", keep_colours=True)
        got = X.refine_device(broken, "shmp", 8, DEV, keep_colours=True, fill=-7).cpu()
        assert got.status.tolist() == host.status.tolist() == [0 if i != where else -1 for i in range(5)]
        ok = np.arange(5) != where
        assert np.array_equal(got.signature[ok], want.signature[ok]) and got.signature[where] == -7
        row_bad = np.concatenate([np.repeat(~ok, np.diff(b.seg_ptr)), ~ok])
        assert (got.colours[row_bad] == -7).all() and np.array_equal(got.colours[~row_bad], want.colours[~row_bad])
    got = X._device(b, X.view_groups("shmp", 4), 8, None, True, DEV, launch_bound=199, fill=-7).cpu()
    assert got.status.tolist() == [0, 0, -1, 0, 0] and got.signature[2] == -7
    assert np.array_equal(np.delete(got.signature, 2), np.delete(want.signature, 2))


# ---- the colour classes against the kernels they claim to bound --------------------------------------------------------
def anchored_batch(pair):
    atlas = R.atlas_connected()
    graphs = [R.anchored_at_largest(atlas[i], a) for i, a in pair]
    gs = GraphSet.from_edge_lists(graphs)
    part = build_partition(gs, 4)
    mine = [k for k in range(part.num_neigh) if part.neigh_index[k, 1] == graphs[part.neigh_index[k, 0]][0] - 1]
    assert len(mine) == 2
    return gs, part, mine


@pytest.fixture(scope="module")
def model():
    nm, _ = make_models(seed=0)                 # 8 layers, H = 64, converted the way main.py converts it
    nm = nm.to(DEV)
    nm.set_queries(standard_queries()[0])
    return nm


def test_a_model_cannot_separate_what_the_classes_merge(model):
    from desco_amd import groundtruth
    gs, part, mine = anchored_batch(R.PAIR_SHMP_BLIND)
    sig = X.refine_device(NeighborhoodBatch(part, DEV), "shmp", 8, DEV).cpu().signature[mine]
    assert sig[0] == sig[1]
    logits = model.graph_to_count(NeighborhoodBatch(part, DEV)).detach()[mine].cpu()
    assert logits.shape[0] == 2 and torch.isfinite(logits).all() and logits.abs().max() > 0
    assert_logits_close("wheel W6 at its hub / apex over two triangles", logits[0:1], logits[1:2], LOGIT_TOL)
    truth = X.neighborhood_truth(gs, X.classes_of(np.asarray(sig), part.neigh_index[mine]), standard_queries()[1],
                                 backend="host")
    assert (truth[0] != truth[1]).any()                                 # ... while the exact counts differ
    floor = X.error_floor(X.classes_of(np.asarray(sig)), truth)
    assert floor.ambiguous_sets.max() == 2 and floor.sse_floor.max() > 0


def test_control_pair_is_not_required_to_agree(model):
    gs, part, mine = anchored_batch(R.PAIR_PLAIN_BLIND)
    batch = NeighborhoodBatch(part, DEV)
    shmp = X.refine_device(batch, "shmp", 8, DEV).cpu().signature[mine]
    plain = X.refine_device(batch, "plain", 8, DEV).cpu().signature[mine]
    assert plain[0] == plain[1] and shmp[0] != shmp[1]                  # only the triangle split tells them apart
    logits = model.graph_to_count(batch).detach()[mine].cpu()
    assert torch.isfinite(logits).all()
    print(f"[control] 250 / 251 under the SHMP model: max |d| / (1 + |ref|) = "
          f"{log_space_err(logits[0:1], logits[1:2]):.2e} (no agreement is required: the classes differ)")
