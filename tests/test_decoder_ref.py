"""CPU side of the decoder feature: the float64 restatement (tests/ref_decoder.py) held to the reference's own outputs in
tests/golden/decoder_golden.npz, the new modules' names and plain spans held to the same fixture, the path selection, the
cache key and the argument checks.  Nothing here needs the GPU or the library."""
import numpy as np
import pytest
import torch

import ref_decoder as RD
from findnpropagate_amd import lib
from findnpropagate_amd.dense_heads import transfusion_decoder as TD
from findnpropagate_amd.model_utils.transfusion_utils import PositionEmbeddingLearned, TransformerDecoderLayer


@pytest.fixture(scope="module")
def golden():
    return np.load(RD.GOLDEN)


def build(name, ffn=None, activation="relu", cross_only=False):
    c = RD.LAYER_CASES[name]
    dec = TransformerDecoderLayer(RD.D, RD.NHEAD, ffn or c["F"], 0.1, activation, self_posembed=PositionEmbeddingLearned(2, RD.D),
                                  cross_posembed=PositionEmbeddingLearned(2, RD.D), cross_only=cross_only)
    heads = TD.SeparateHead_Transfusion(RD.D, 64, 1, RD.sep_head_dict(c["heads"]), use_bias=c["bias"])
    if ffn is None and not cross_only:
        dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in RD.decoder_weights(c["seed"], c["F"]).items()}, strict=True)
    heads.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in RD.head_weights(c["seed"], c["heads"], c["bias"]).items()}, strict=True)
    return dec.eval(), heads.eval()


def inputs(name):
    c = RD.LAYER_CASES[name]
    query, key, query_pos, bev_pos = (torch.from_numpy(a) for a in RD.layer_inputs(name))
    return query, key, query_pos, bev_pos.repeat(c["B"], 1, 1)


@pytest.mark.parametrize("name", list(RD.LAYER_CASES))
def test_restatement_matches_reference_layer(golden, name):
    assert golden[name + "_crc"].tolist() == [RD.crc(a) for a in RD.layer_inputs(name)], "the generators no longer give the fixture's inputs"
    want = RD.layer_case64(name)
    for k in list(RD.LAYER_CASES[name]["heads"]) + ["query_feat"]:
        err = float(golden[f"{name}_err_{k}"][0])
        got = RD.rel_err(golden[f"{name}_{k}"], want[k])
        print(name, k, got, err)
        assert 0 < err < 2e-6 and got <= err * (1 + 1e-6)


@pytest.mark.parametrize("name", list(RD.ATT_CASES))
def test_restatement_matches_reference_attention(golden, name):
    assert golden[name + "_crc"].tolist() == [RD.crc(a) for a in RD.attention_inputs(name)]
    err = float(golden[name + "_err_out"][0])
    assert 0 < err < 2e-6 and RD.rel_err(golden[name + "_out"], RD.attention_case64(name)) <= err * (1 + 1e-6)


def test_end_to_end_fixture_is_decided_by_margins(golden):
    assert golden["e2e_crc"].tolist() == [RD.crc(a) for a in RD.e2e_inputs()]
    keep, s64, b64 = golden["e2e_keep"], golden["e2e_scores64"], golden["e2e_boxes64"]
    lim = np.asarray(RD.E2E_POST["POST_CENTER_RANGE"])
    mine = (s64 > RD.E2E_POST["SCORE_THRESH"]) & (b64[..., :3] >= lim[:3]).all(-1) & (b64[..., :3] <= lim[3:]).all(-1)
    assert np.array_equal(mine, keep) and 0 < keep.sum() < keep.size
    assert np.abs(s64 - RD.E2E_POST["SCORE_THRESH"]).min() > 8 * float(golden["e2e_err_score"][0]) * np.abs(s64).max()
    assert np.abs(b64[..., 0] - lim[0]).min() > 8 * float(golden["e2e_err_center"][0]) * np.abs(b64[..., :2]).max()


def test_state_dict_names_and_shapes(golden):
    dec, heads = build("mid")
    for tag, m in (("decoder", dec), ("heads", heads)):
        sd = m.state_dict()
        assert list(sd) == golden[tag + "_keys"].tolist()
        assert ["x".join(str(s) for s in v.shape) for v in sd.values()] == golden[tag + "_shapes"].tolist()


@pytest.mark.parametrize("name", list(RD.LAYER_CASES))
def test_plain_spans_match_reference(golden, name):
    dec, heads = build(name)
    query, key, query_pos, bev_pos = inputs(name)
    with torch.no_grad():
        x = dec.forward_plain(query, key, query_pos, bev_pos)
        res = TD.DecoderHead(dec, heads).call_plain(query, key, query_pos, bev_pos)
        assert torch.equal(dec(query, key, query_pos, bev_pos), x)          # CPU tensors: forward is the plain span
    res["query_feat"] = x
    for k, v in res.items():
        want = golden[f"{name}_{k}"].astype(np.float64)
        got = RD.rel_err(v.numpy(), want)
        print(name, k, got)
        assert got <= RD.TOL_FACTOR * float(golden[f"{name}_err_{k}"][0])


def test_geometry_rule():
    assert RD.attention_geometry(32400) == (512, 64)
    assert RD.attention_geometry(200) == (256, 64) and RD.attention_geometry(7) == (256, 64)
    assert RD.attention_geometry(64 * 256 + 1) == (320, 64)
    assert -(-32400 // 512) * RD.NHEAD >= 256         # one scene gives a workgroup per CU


def test_path_selection(monkeypatch):
    def no_library():
        raise AssertionError("the plain span must not touch the library")

    monkeypatch.setattr(lib, "load", no_library)
    dec, heads = build("tiny")
    query, key, query_pos, bev_pos = inputs("tiny")
    args = (query, key, query_pos, bev_pos)
    with torch.no_grad():
        want = dec.forward_plain(*args)
        assert dec.plain_reasons(*args) == ["not on the device"]             # everything else is in favour
        assert torch.equal(dec(*args), want)
        mask = torch.zeros(1, key.shape[2], dtype=torch.bool)
        assert "mask" in dec.plain_reasons(*args, key_padding_mask=mask) and "mask" in dec.plain_reasons(*args, attn_mask=torch.zeros(5, 9))
        assert torch.equal(dec(*args, key_padding_mask=mask), want)
        assert "dtype" in dec.plain_reasons(query.double(), key, query_pos, bev_pos)
        assert "autograd" not in dec.plain_reasons(*args)
    assert "autograd" in dec.plain_reasons(*args)                            # recording, and the parameters require grad
    for p in dec.parameters():
        p.requires_grad_(False)
    assert "autograd" not in dec.plain_reasons(*args)
    assert "autograd" in dec.plain_reasons(query.clone().requires_grad_(), key, query_pos, bev_pos)
    dec.train()
    assert "training mode" in dec.plain_reasons(*args)
    torch.manual_seed(3)
    a = dec(*args)
    torch.manual_seed(3)
    assert torch.equal(a, dec.forward_plain(*args))
    with torch.no_grad():
        for kw, reason in ((dict(ffn=24), "dim_feedforward"), (dict(ffn=2048), "dim_feedforward"), (dict(activation="gelu"), "activation"),
                           (dict(cross_only=True), "cross_only")):
            other = build("tiny", **kw)[0]
            assert reason in other.plain_reasons(*args), reason
            other(*args)
        wide = TransformerDecoderLayer(64, 8, 32, self_posembed=PositionEmbeddingLearned(2, 64), cross_posembed=PositionEmbeddingLearned(2, 64)).eval()
        assert "d_model / nhead" in wide.plain_reasons(*args)
        four = TransformerDecoderLayer(RD.D, 4, 32, self_posembed=PositionEmbeddingLearned(2, RD.D), cross_posembed=PositionEmbeddingLearned(2, RD.D)).eval()
        assert "d_model / nhead" in four.plain_reasons(*args)                # d_model 128 with other than 8 heads
        assert four(*args).shape == want.shape
        bare = TransformerDecoderLayer(RD.D, RD.NHEAD, 32).eval()
        assert "position embedding" in bare.plain_reasons(*args)
        # the heads: a 3-wide kernel, three convolutions or a missing center head pick the plain span
        assert TD.heads_plain_reasons(heads) == ["not on the device"]
        k3 = TD.SeparateHead_Transfusion(RD.D, 64, 3, RD.sep_head_dict(RD.NUSC_HEADS)).eval()
        assert any("head layout" in r for r in TD.heads_plain_reasons(k3))
        deep = TD.SeparateHead_Transfusion(RD.D, 64, 1, {"center": dict(out_channels=2, num_conv=3)}).eval()
        assert any("head layout" in r for r in TD.heads_plain_reasons(deep))
        res = TD.DecoderHead(dec.eval(), k3)(*args)
        assert res["center"].shape == (1, 2, 5)
        # what a cache key cannot see: a submodule alone in train(), a BatchNorm without running statistics, a half-precision buffer
        fresh, fresh_heads = build("tiny")
        bn = fresh.cross_posembed.position_embedding_head[1]
        bn.train()
        assert "training mode" in fresh.plain_reasons(*args)
        bn.eval()
        assert "training mode" not in fresh.plain_reasons(*args)
        bn.running_var = bn.running_var.half()
        assert "dtype" in fresh.plain_reasons(*args)
        bn._buffers["running_var"] = None
        assert "position embedding" in fresh.plain_reasons(*args)
        fresh_heads.center[0][1]._buffers["running_mean"] = None
        assert any("head layout" in r for r in TD.heads_plain_reasons(fresh_heads))


def test_copies_and_pickles_travel_without_the_device_cache():
    import copy
    import pickle

    dec, _ = build("tiny")
    args = inputs("tiny")
    with torch.no_grad():
        want = dec(*args)
        assert dec._device_pack is not None
        for other in (copy.deepcopy(dec), pickle.loads(pickle.dumps(dec))):
            assert other._device_pack is None and dec._device_pack is not None
            assert torch.equal(other(*args), want)


def test_cache_key_follows_every_slot():
    dec, heads = build("tiny")
    bev_pos = inputs("tiny")[3]
    key = lambda: TD.cache_key(dec, heads, bev_pos)
    k0 = key()
    assert key() == k0
    with torch.no_grad():
        dec.multihead_attn.in_proj_weight.add_(0.5)
    k1 = key()
    assert k1 != k0
    dec.load_state_dict(dec.state_dict())
    k2 = key()
    assert k2 != k1
    with torch.no_grad():
        heads.center[0][1].running_var.mul_(2.0)
    k3 = key()
    assert k3 != k2
    bn = dec.cross_posembed.position_embedding_head[1]
    bn._buffers["running_mean"] = None
    k4 = key()
    assert k4 != k3 and len(k4) == len(k3)                # the empty slot is part of the key
    bn.running_mean = torch.zeros(RD.D)
    k5 = key()
    assert k5 != k4
    with torch.no_grad():
        bev_pos.add_(1.0)
    assert key() != k5
    assert TD.cache_key(dec, heads, bev_pos.clone()) != key()


def test_argument_checks():
    q, k, v = torch.zeros(1, 5, 128), torch.zeros(1, 9, 128), torch.zeros(1, 9, 128)
    assert TD.check_attention(q, k, v) == (1, 5, 9)
    for bad in ((q.double(), k, v), (q[:, :, :64], k, v), (q, k, v[:, :8]), (torch.zeros(2, 5, 128), k, v), (torch.zeros(1, 2049, 128), k, v),
                (q, torch.zeros(1, 0, 128), torch.zeros(1, 0, 128)), (q[0], k, v)):
        with pytest.raises(AssertionError):
            TD.check_attention(*bad)
    with pytest.raises(lib.FnpError):
        TD.attention(q, k, v)                              # CPU tensors: there is no CPU path
