"""Neighborhood models of other widths than 64 (--neigh_hidden_dim != 64), host side: construction with the reference's
state-dict names and true shapes, the refusals, and the exactness of the per-block zero padding (CPU oracle)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from desco_amd import gnn_model as GM  # noqa: E402
from oracle import model as OM  # noqa: E402
from oracle import partition as OP  # noqa: E402

from helpers import cpu_sd, golden_graphs, gossip_args, neigh_args, standard_queries  # noqa: E402


def width_models(h, seed=0, tconv=True, layer_num=3):
    from desco_amd.lightning_model import GossipCountingModel, NeighborhoodCountingModel
    torch.manual_seed(seed)
    nm = NeighborhoodCountingModel(1, h, neigh_args(hidden_dim=h, layer_num=layer_num, use_tconv=tconv))
    nm.to_hetero_old(tconv, tconv)
    gm = GossipCountingModel(1, 64, gossip_args(), emb_channels=h, input_pattern_emb=True)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m, gain in ((nm, 1.3), (gm, 1.4)):
            for _, p in m.named_parameters():
                if p.dim() == 2:
                    p.mul_(gain)
                else:
                    p.add_(0.1 * torch.randn(p.shape, generator=g))
    return nm, gm


def padded_state_dict(nm):
    """The state dict of the same model at width wp = padded_width(h), every h-wide block zero-padded on its own with
    the packer's helpers (gnn_model._pad_blocks / _pad_to)."""
    h = nm.hidden_dim
    wp = GM.padded_width(h)
    L = nm.emb_model.gnn_core.layer_num
    out = {}
    for k, v in cpu_sd(nm).items():
        v = v.clone()
        if k.startswith("count_model.0.weight"):
            vt = torch.nn.functional.pad(v.view(v.shape[0], 2, h), (0, wp - h)).view(v.shape[0], 2 * wp)
            v = GM._pad_to(vt, 4 * wp, 2 * wp)
        elif k in ("count_model.0.bias", "count_model.2.weight"):
            v = GM._pad_to(v, *([4 * wp] if v.dim() == 1 else [1, 4 * wp]))
        elif k == "count_model.2.bias":
            pass
        elif "anchor_mlp.0" in k:
            v = GM._pad_blocks(v, h, wp, L + 1, L + 1) if v.dim() == 2 else \
                torch.nn.functional.pad(v.view(L + 1, h), (0, wp - h)).reshape(-1)
        elif "post_mp.0" in k:
            v = GM._pad_to(torch.nn.functional.pad(v.view(h, L + 1, h), (0, wp - h)).reshape(h, -1), wp, (L + 1) * wp) \
                if v.dim() == 2 else GM._pad_to(v, wp)
        elif "post_mp." in k:
            v = GM._pad_to(v, *[GM.padded_width(d) for d in v.shape])
        elif "updates" in k:
            v = GM._pad_blocks(v, h, wp, 1, 2) if v.dim() == 2 else GM._pad_to(v, wp)
        elif "pre_mp" in k:
            v = GM._pad_to(v, wp, v.shape[1]) if v.dim() == 2 else GM._pad_to(v, wp)
        elif "convs" in k:
            v = GM._pad_to(v, wp, wp) if v.dim() == 2 else GM._pad_to(v, wp)
        else:
            raise AssertionError(f"unexpected key {k}")
        out[k] = v
    return out


@pytest.mark.parametrize("h", [32, 100, 128, 256])
def test_models_build_with_reference_names_and_true_shapes(h):
    nm, gm = width_models(h, layer_num=8)
    ref, _ = width_models(64, layer_num=8)
    sd, sd64 = nm.state_dict(), ref.state_dict()
    assert list(sd) == list(sd64)
    head = {"count_model.0.weight": (4 * h, 2 * h), "count_model.0.bias": (4 * h,), "count_model.2.weight": (1, 4 * h),
            "count_model.2.bias": (1,)}
    scale = lambda d: d if d in (1, 256) else d // 64 * h     # noqa: E731  (64-multiples scale with the width)
    for k, v in sd.items():
        want = head.get(k, tuple(scale(d) for d in sd64[k].shape))
        assert tuple(v.shape) == want, (k, tuple(v.shape))
    assert gm.emb_model.gnn_core.convs[0].lin_gate[0].in_features == h
    assert gm.emb_model.post_mp[0].in_features == h + 64 * 3
    pk = GM.pack_shmp_wide(nm.emb_model, planes=False)
    wp = GM.padded_width(h)
    assert pk["wp"] == wp and pk["layers"][0]["count"]["wt"].shape == (5 * wp, wp)
    assert pk["anchor"][0].shape == (9 * wp, 9 * wp) and pk["post"][0][0].shape == (9 * wp, wp)


def test_refusals_name_the_flag():
    from desco_amd.lightning_model import GossipCountingModel, NeighborhoodCountingModel
    with pytest.raises(NotImplementedError, match="--gossip_hidden_dim"):
        GossipCountingModel(1, 128, gossip_args(hidden_dim=128), emb_channels=64, input_pattern_emb=True)
    with pytest.raises(NotImplementedError, match=r"--neigh_hidden_dim must be in 1\.\.256"):
        NeighborhoodCountingModel(1, 300, neigh_args(hidden_dim=300))
    with pytest.raises(NotImplementedError, match="--neigh_hidden_dim"):
        GossipCountingModel(1, 64, gossip_args(), emb_channels=300, input_pattern_emb=True)


@pytest.mark.parametrize("h", [32, 100])
def test_per_block_zero_padding_is_exact_on_the_oracle(h):
    """The oracle on the state dict padded block by block to wp equals the oracle on the true one: logits of the
    neighborhood model and the query embeddings (padded channels exactly 0)."""
    nm, _ = width_models(h)
    qids, queries = standard_queries()
    graphs = golden_graphs(max_n=30)[:6]
    _, _, neighs = OP.neighborhood_dataset(graphs, 4)
    ob, qb = OP.neighborhood_batch(neighs), OP.query_batch(queries)
    sd, sdp = cpu_sd(nm), padded_state_dict(nm)
    ref = OM.neighborhood_logits(sd, ob, qb, layer_num=3, emulate_quirk=False)[0]
    got = OM.neighborhood_logits(sdp, ob, qb, layer_num=3, emulate_quirk=False)[0]
    d = float((got - ref).abs().max())
    print(f"[gate] padded-vs-true oracle logits at h={h}: max |d| = {d:.2e} (gate 1e-6)")
    assert d <= 1e-6
    qe = OM.neighborhood_embed_queries(sd, qb, 3)
    qep = OM.neighborhood_embed_queries(sdp, qb, 3)
    assert float((qep[:, :h] - qe).abs().max()) <= 1e-6 and float(qep[:, h:].abs().max()) == 0.0


@pytest.mark.parametrize("h", [32, 100])
def test_packer_layout_is_that_of_the_padded_model(h):
    """pack_shmp_wide of the width-h model equals pack_shmp_wide of the width-wp model holding the padded state dict
    (whose oracle equals the true one: test above), operand for operand -- both models and the count head."""
    from desco_amd.lightning_model import NeighborhoodCountingModel
    nm, _ = width_models(h)
    wp = GM.padded_width(h)
    big = NeighborhoodCountingModel(1, wp, neigh_args(hidden_dim=wp, layer_num=3)).to_hetero_old(True, True)
    big.load_state_dict(padded_state_dict(nm))

    def close(name, a, b):
        assert a.shape == b.shape, (name, tuple(a.shape), tuple(b.shape))
        d = float((a - b).abs().max()) if a.numel() else 0.0
        assert d <= 1e-6 * (1.0 + float(b.abs().max())), (name, d)

    for m, mb in ((nm.emb_model, big.emb_model), (nm.emb_model_query, big.emb_model_query)):
        with torch.no_grad():
            pk, pkb = GM.pack_shmp_wide(m, planes=False), GM.pack_shmp_wide(mb, planes=False)
        for t in pk["pre"]:
            for i in range(2):
                close(f"pre {t}", pk["pre"][t][i], pkb["pre"][t][i])
        for l, (e, eb) in enumerate(zip(pk["layers"], pkb["layers"])):
            for t in e:
                close(f"layer {l} {t} wt", e[t]["wt"], eb[t]["wt"])
                close(f"layer {l} {t} b", e[t]["b"], eb[t]["b"])
        if "anchor" in pk:
            for i in range(2):
                close("anchor", pk["anchor"][i], pkb["anchor"][i])
        for j in range(4):
            for i in range(2):
                close(f"post {j}", pk["post"][j][i], pkb["post"][j][i])
    with torch.no_grad():       # (the head's hidden width: padded_width(4 h) against 4 wp -- the rest is zero)
        for a, b in zip(nm._head_wide_operands(), big._head_wide_operands()):
            n = a.shape[-1]
            close("count head", a, b[..., :n])
            assert float(b[..., n:].abs().max()) == 0.0 if b.shape[-1] > n else True
