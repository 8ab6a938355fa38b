"""The decoder layer and the prediction heads on the device (csrc/tfdecoder.hip) against exact constructions (one-hot and
uniform attention), against themselves (batch independence, run-to-run bits) and against the float64 restatement of
tests/ref_decoder.py within TOL_FACTOR = 4 x the reference's own f32 error recorded in tests/golden/decoder_golden.npz.

Measured on one MI355X (max |device - f64| / max |f64| over the fixture's err; allowed 4): attention alone 1.45-1.71, layer and
heads 0.66-1.70 on the 437- and 32,400-cell cases, largest 2.97 (`height` of the 5-query, 9-cell case), K = 300 1.08, end to end
centres 0.73 and scores 1.00; uniform attention within 0.50 ulp of the f64 mean."""
import numpy as np
import pytest
import torch

import ref_decoder as RD
from findnpropagate_amd.dense_heads import transfusion_decoder as TD
from findnpropagate_amd.model_utils.transfusion_utils import PositionEmbeddingLearned, TransformerDecoderLayer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(RD.GOLDEN)


def build(name, dev):
    c = RD.LAYER_CASES[name]
    dec = TransformerDecoderLayer(RD.D, RD.NHEAD, c["F"], 0.1, "relu", self_posembed=PositionEmbeddingLearned(2, RD.D),
                                  cross_posembed=PositionEmbeddingLearned(2, RD.D))
    heads = TD.SeparateHead_Transfusion(RD.D, 64, 1, RD.sep_head_dict(c["heads"]), use_bias=c["bias"])
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in RD.decoder_weights(c["seed"], c["F"]).items()}, strict=True)
    heads.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in RD.head_weights(c["seed"], c["heads"], c["bias"]).items()}, strict=True)
    return dec.eval().to(dev), heads.eval().to(dev)


def inputs(name, dev):
    return tuple(torch.from_numpy(a).to(dev) for a in RD.layer_inputs(name))


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. one-hot attention, exact ---------------------------------------------------------------------------------------------


def border_keys(n):
    split_len, tile_len = TD.attention_geometry(n)
    assert (split_len, tile_len) == RD.attention_geometry(n)
    keys = {0, n - 1}
    for step in (split_len, tile_len):
        for edge in range(step, n, step):
            keys |= {edge - 1, edge}
    return sorted(keys)


@pytest.mark.parametrize("B,Kq,N", [(1, 5, 7), (2, 37, 437), (2, 37, None)])
def test_one_hot_attention_is_exact(cuda, B, Kq, N):
    if N is None:
        N = 3 * RD.attention_geometry(437)[0] + 5
    rng = np.random.default_rng(N)
    special = border_keys(N) if N > 16 else list(range(N))
    q = np.zeros((B, Kq, RD.D), np.float32)
    k = np.zeros((B, N, RD.D), np.float32)
    v = rng.normal(0, 1, (B, N, RD.D)).astype(np.float32)
    chosen = np.zeros((B, Kq, RD.NHEAD), np.int64)
    for b in range(B):
        for h in range(RD.NHEAD):
            mine = [special[(16 * h + 5 * b + j) % len(special)] for j in range(min(16, len(special)))]
            mine = list(dict.fromkeys(mine))                       # a head's keys, each with a dimension of its own
            for d, n in enumerate(mine):
                k[b, n, 16 * h + d] = 16.0
            for j in range(Kq):
                d = (j + h) % len(mine)                            # a different key per head of one query
                q[b, j, 16 * h + d] = 32.0                         # 0.25 * 32 * 16 = 128 against 0: exp(-128) is 0 in f32
                chosen[b, j, h] = mine[d]
    used = set(chosen.ravel().tolist())
    if Kq >= 16:
        assert set(special) <= used and {0, N - 1} <= used, "every border key is some query's chosen key"
    out = torch.full((B, Kq, RD.D), float("nan"), device=cuda)
    TD.attention(torch.from_numpy(q).to(cuda), torch.from_numpy(k).to(cuda), torch.from_numpy(v).to(cuda), out=out)
    want = np.empty_like(q)
    for b in range(B):
        for j in range(Kq):
            for h in range(RD.NHEAD):
                want[b, j, 16 * h:16 * h + 16] = v[b, chosen[b, j, h], 16 * h:16 * h + 16]
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))


# ---- 2. uniform attention: every key counted once ---------------------------------------------------------------------------


@pytest.mark.parametrize("N", [437, 32400])
@pytest.mark.parametrize("Kq", [16, 17, 200])
def test_uniform_attention_counts_every_key(cuda, N, Kq):
    rng = np.random.default_rng(N + Kq)
    v = rng.integers(1, 65, (1, N, RD.D)).astype(np.float32)
    k = rng.normal(0, 1, (1, N, RD.D)).astype(np.float32)
    out = TD.attention(torch.zeros((1, Kq, RD.D), device=cuda), torch.from_numpy(k).to(cuda), torch.from_numpy(v).to(cuda)).cpu().numpy()
    mean = v[0].astype(np.float64).mean(0)
    ulp = np.spacing(mean.astype(np.float32)).astype(np.float64)
    worst = float((np.abs(out[0].astype(np.float64) - mean) / ulp).max())
    print("uniform attention", N, Kq, "worst", worst, "ulp")
    assert worst <= 2.0


# ---- 3. batch independence and run-to-run bits ------------------------------------------------------------------------------


def test_attention_batch_independence(cuda):
    rng = np.random.default_rng(5)
    q, k, v = (torch.from_numpy(rng.normal(0, 1, s).astype(np.float32)).to(cuda) for s in ((3, 37, 128), (3, 437, 128), (3, 437, 128)))
    whole = TD.attention(q, k, v)
    assert torch.equal(bits(whole), bits(TD.attention(q, k, v)))
    for b in range(3):
        alone = TD.attention(q[b:b + 1], k[b:b + 1], v[b:b + 1])
        assert torch.equal(bits(alone[0]), bits(whole[b])), b


def test_decoder_head_batch_independence(cuda):
    dec, heads = build("mid", cuda)
    rng = np.random.default_rng(6)
    N = 23 * 19
    query = torch.from_numpy(rng.normal(0, 1, (3, 128, 37)).astype(np.float32)).to(cuda)
    key = torch.from_numpy(rng.normal(0, 1, (3, 128, N)).astype(np.float32)).to(cuda)
    bev_pos = inputs("mid", cuda)[3]
    query_pos = bev_pos[0][torch.from_numpy(rng.integers(0, N, (3, 37))).to(cuda)]
    head = TD.DecoderHead(dec, heads)
    with torch.no_grad():
        assert head.plain_reasons(query, key, query_pos, bev_pos) == []
        whole = head(query, key, query_pos, bev_pos)
        again = head(query, key, query_pos, bev_pos)
        for name in whole:
            assert torch.equal(bits(whole[name]), bits(again[name])), name
        for b in range(3):
            alone = head(query[b:b + 1], key[b:b + 1], query_pos[b:b + 1], bev_pos)
            for name in whole:
                assert torch.equal(bits(alone[name][0]), bits(whole[name][b])), (name, b)


# ---- 4. random cases against the fixture ------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(RD.ATT_CASES))
def test_attention_against_fixture(cuda, golden, name):
    q, k, v = (torch.from_numpy(a).to(cuda) for a in RD.attention_inputs(name))
    got = TD.attention(q, k, v).cpu().numpy()
    err = float(golden[name + "_err_out"][0])
    ratio = RD.rel_err(got, RD.attention_case64(name)) / err
    print(f"attention {name}: device error / reference error = {ratio:.3f}")
    assert ratio <= RD.TOL_FACTOR


@pytest.mark.parametrize("name", list(RD.LAYER_CASES))
def test_layer_and_heads_against_fixture(cuda, golden, name):
    dec, heads = build(name, cuda)
    query, key, query_pos, bev_pos = inputs(name, cuda)
    want = RD.layer_case64(name)
    with torch.no_grad():
        assert dec.plain_reasons(query, key, query_pos, bev_pos) == []
        x = dec(query, key, query_pos, bev_pos)
        res = dict(TD.DecoderHead(dec, heads)(query, key, query_pos, bev_pos))
    assert x.shape == want["query_feat"].shape and set(res) == set(RD.LAYER_CASES[name]["heads"])
    res["query_feat"] = x
    worst = 0.0
    for k, t in res.items():
        assert t.is_contiguous() and t.shape == want[k].shape
        ratio = RD.rel_err(t.cpu().numpy(), want[k]) / float(golden[f"{name}_err_{k}"][0])
        print(f"layer {name} {k}: device error / reference error = {ratio:.3f}")
        worst = max(worst, ratio)
    assert worst <= RD.TOL_FACTOR


# ---- 5. fallbacks on the device ---------------------------------------------------------------------------------------------


def test_fallbacks_on_the_device(cuda):
    dec, heads = build("mid", cuda)
    query, key, query_pos, bev_pos = inputs("mid", cuda)
    bev_b = bev_pos.repeat(2, 1, 1)
    with torch.no_grad():
        plain = dec.forward_plain(query, key, query_pos, bev_b)
        mask = torch.zeros((2, key.shape[2]), dtype=torch.bool, device=cuda)
        assert torch.equal(dec(query, key, query_pos, bev_b, key_padding_mask=mask), dec.forward_plain(query, key, query_pos, bev_b, key_padding_mask=mask))
        device = dec(query, key, query_pos, bev_b)
        assert not torch.equal(device, plain) and torch.allclose(device, plain, atol=1e-4)     # the two paths are different code
    q2 = query.clone().requires_grad_()
    out = dec(q2, key, query_pos, bev_b)
    assert torch.equal(out.detach(), plain)
    out.square().sum().backward()
    assert q2.grad is not None and torch.isfinite(q2.grad).all() and dec.linear1.weight.grad is not None
    res = TD.DecoderHead(dec, heads)(q2, key, query_pos, bev_b)
    res["center"].sum().backward()
    dec.train()
    torch.manual_seed(11)
    a = dec(query, key, query_pos, bev_b)
    torch.manual_seed(11)
    assert torch.equal(a, dec.forward_plain(query, key, query_pos, bev_b))


# ---- 6. the cache follows in-place changes ----------------------------------------------------------------------------------


def test_cache_follows_weights_and_positions(cuda, golden):
    name = "mid"
    c = RD.LAYER_CASES[name]
    dec, heads = build(name, cuda)
    query, key, query_pos, bev_pos = inputs(name, cuda)
    sd = RD.decoder_weights(c["seed"], c["F"])
    err = float(golden[f"{name}_err_query_feat"][0])
    with torch.no_grad():
        first = dec(query, key, query_pos, bev_pos)
        dec.multihead_attn.in_proj_weight[RD.D:].mul_(1.25)                  # the key and value projections
        sd["multihead_attn.in_proj_weight"] = sd["multihead_attn.in_proj_weight"].copy()
        sd["multihead_attn.in_proj_weight"][RD.D:] *= np.float32(1.25)
        second = dec(query, key, query_pos, bev_pos)
        want = RD.layer64(sd, *RD.layer_inputs(name))
        assert not torch.equal(first, second)
        ratio = RD.rel_err(second.cpu().numpy(), want) / err
        print(f"after the weight update: {ratio:.3f}")
        assert ratio <= RD.TOL_FACTOR
        bev_pos.mul_(0.5)
        third = dec(query, key, query_pos, bev_pos)
        q_np, k_np, qp_np, bp_np = RD.layer_inputs(name)
        want = RD.layer64(sd, q_np, k_np, qp_np, bp_np * np.float32(0.5))
        assert not torch.equal(second, third)
        ratio = RD.rel_err(third.cpu().numpy(), want) / err
        print(f"after the position update: {ratio:.3f}")
        assert ratio <= RD.TOL_FACTOR


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------


def test_end_to_end_against_reference_predict_and_get_bboxes(cuda, golden):
    from findnpropagate_amd.dense_heads.transfusion_proposals import BoxDecoder, HeatmapProposals

    c = RD.E2E
    B, C, K, N = c["B"], c["C"], c["K"], c["H"] * c["W"]
    assert golden["e2e_crc"].tolist() == [RD.crc(a) for a in RD.e2e_inputs()]
    logits, feat, enc_w, enc_b = (torch.from_numpy(a).to(cuda) for a in RD.e2e_inputs())
    dec, heads = build_e2e(cuda)
    table = torch.from_numpy(RD.create_2d_grid(c["W"], c["H"])[0]).to(cuda)          # the head's bev_pos, rows as create_2D_grid
    bev_xy = table.flip(dims=[-1])[None].contiguous()
    proposals = HeatmapProposals(K, 3, C, "nuScenes")
    boxdec = BoxDecoder(RD.E2E_POST, RD.E2E_STRIDE, RD.E2E_VOXEL, RD.E2E_PCR, C)
    with torch.no_grad():
        top_class, top_index, _, qhs = proposals(logits)
        flat = feat.view(B, RD.D, N)
        query_feat, query_pos = proposals.init_queries(flat, table, enc_w, enc_b, top_class, top_index)
        head = TD.DecoderHead(dec, heads)
        assert head.plain_reasons(query_feat, flat, query_pos, bev_xy) == []
        res = head(query_feat, flat, query_pos, bev_xy)
        kept = boxdec.get_bboxes({**res, "query_heatmap_score": qhs}, top_class)     # the path INTEGRATION section 2 patches in
    assert np.array_equal(top_class.cpu().numpy(), golden["e2e_query_labels"])
    keep = golden["e2e_keep"]
    assert len(kept) == B and [int(d["pred_boxes"].shape[0]) for d in kept] == keep.sum(1).tolist()
    all64 = golden["e2e_boxes64"]
    scale_c, scale_s = np.abs(all64[..., :2]).max(), np.abs(golden["e2e_scores64"]).max()
    tol_c = RD.TOL_FACTOR * float(golden["e2e_err_center"][0]) * scale_c
    worst_c = worst_s = 0.0
    for b in range(B):
        boxes, scores, labels = (kept[b][k].cpu().numpy() for k in ("pred_boxes", "pred_scores", "pred_labels"))
        assert boxes.shape[1] == 9
        # the kept SET and its order: every returned row is matched to the one query of the scene whose f64 centre it meets
        # (the proposals sit in distinct cells, so centres are far apart), and those queries are the reference's, in its order
        dist = np.abs(boxes[:, None, :2].astype(np.float64) - all64[b][None, :, :2]).max(-1)
        assert ((dist <= tol_c).sum(1) == 1).all()
        assert np.array_equal(dist.argmin(1), np.nonzero(keep[b])[0])
        want_boxes, want_scores = all64[b][keep[b]], golden["e2e_scores64"][b][keep[b]]
        assert np.array_equal(labels, golden["e2e_labels"][b][keep[b]])
        worst_c = max(worst_c, float(np.abs(boxes[:, :2].astype(np.float64) - want_boxes[:, :2]).max() / scale_c))
        worst_s = max(worst_s, float(np.abs(scores.astype(np.float64) - want_scores).max() / scale_s))
    ratio_c, ratio_s = worst_c / float(golden["e2e_err_center"][0]), worst_s / float(golden["e2e_err_score"][0])
    print(f"end to end: centres {ratio_c:.3f}, scores {ratio_s:.3f} of the reference's own error")
    assert ratio_c <= RD.TOL_FACTOR and ratio_s <= RD.TOL_FACTOR


def test_fallbacks_the_key_cannot_see(cuda):
    """a module state the device path cannot serve must pick the plain span, not raise: no running statistics in a position
    embedding's BatchNorm, a submodule alone left in train(), a buffer off the device"""
    name = "tiny"
    query, key, query_pos, bev_pos = inputs(name, cuda)
    with torch.no_grad():
        dec, heads = build(name, cuda)
        bn = dec.cross_posembed.position_embedding_head[1]
        bn._buffers["running_mean"] = None
        assert "position embedding" in dec.plain_reasons(query, key, query_pos, bev_pos)
        dec, heads = build(name, cuda)
        want = dec(query, key, query_pos, bev_pos)
        dec.self_posembed.position_embedding_head[1].train()
        assert "training mode" in dec.plain_reasons(query, key, query_pos, bev_pos)
        dec.eval()
        assert dec.plain_reasons(query, key, query_pos, bev_pos) == []
        dec.self_posembed.position_embedding_head[1].running_var = dec.self_posembed.position_embedding_head[1].running_var.cpu()
        assert "not on the device" in dec.plain_reasons(query, key, query_pos, bev_pos)
        dec.self_posembed.position_embedding_head[1].running_var = dec.self_posembed.position_embedding_head[1].running_var.to(cuda)
        assert torch.equal(dec(query, key, query_pos, bev_pos), want)
        heads.center[0][1]._buffers["running_var"] = None
        assert any("head layout" in r for r in TD.DecoderHead(dec, heads).plain_reasons(query, key, query_pos, bev_pos))


def build_e2e(dev):
    c = RD.E2E
    dec = TransformerDecoderLayer(RD.D, RD.NHEAD, c["F"], 0.1, "relu", self_posembed=PositionEmbeddingLearned(2, RD.D),
                                  cross_posembed=PositionEmbeddingLearned(2, RD.D))
    heads = TD.SeparateHead_Transfusion(RD.D, 64, 1, RD.sep_head_dict(c["heads"]), use_bias=c["bias"])
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in RD.decoder_weights(c["seed"], c["F"]).items()}, strict=True)
    heads.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in RD.head_weights(c["seed"], c["heads"], c["bias"]).items()}, strict=True)
    return dec.eval().to(dev), heads.eval().to(dev)


def test_more_than_256_queries_take_the_merged_self_attention(cuda):
    """K = 300: the self-attention has two splits and a merge launch of its own (eight launches), and two query chunks per
    head.  The yardstick is made here: the plain span on the CPU in f32 (the reference's ops, held to the fixture by
    tests/test_decoder_ref.py) against the f64 restatement gives the reference's own error on these inputs."""
    c = RD.LAYER_CASES["mid"]
    rng = np.random.default_rng(77)
    K, N = 300, c["H"] * c["W"]
    assert RD.attention_geometry(K)[0] < K
    dec, _ = build("mid", torch.device("cpu"))
    bev = RD.layer_inputs("mid")[3]
    query = rng.normal(0, 1, (1, RD.D, K)).astype(np.float32)
    key = rng.normal(0, 1, (1, RD.D, N)).astype(np.float32)
    query_pos = bev[0][rng.integers(0, N, (1, K))]
    want = RD.layer64(RD.decoder_weights(c["seed"], c["F"]), query, key, query_pos, bev)
    with torch.no_grad():
        plain = dec.forward_plain(*(torch.from_numpy(a) for a in (query, key, query_pos, bev)))
        err = RD.rel_err(plain.numpy(), want)
        dec = dec.to(cuda)
        args = tuple(torch.from_numpy(a).to(cuda) for a in (query, key, query_pos, bev))
        assert dec.plain_reasons(*args) == []
        got = dec(*args)
    ratio = RD.rel_err(got.cpu().numpy(), want) / err
    print(f"K = 300: device error / plain f32 error = {ratio:.3f} (plain f32 error {err:.3e})")
    assert 1e-8 < err < 2e-6 and ratio <= RD.TOL_FACTOR
