"""The yardstick of the attention-dropout tests (tests/ref_attention_dropout.py) held to what stands outside the project: its
Philox core to the published known-answer vectors, its float64 statement to torch's float64 autograd of the same masked
expression, its mask to the statistics of independent bits; and what the dropout arguments and the decoder layer's
fused_attention_dropout attribute decide on the host (no GPU)."""
import numpy as np
import pytest
import torch

import ref_attention_dropout as RA
import ref_attention_grad as RG
import ref_decoder as RD
from findnpropagate_amd.dense_heads import transfusion_decoder as TD
from findnpropagate_amd.model_utils.transfusion_utils import PositionEmbeddingLearned, TransformerDecoderLayer

KNOWN_ANSWERS = [            # Random123's kat_vectors for philox4x32 with ten rounds: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_philox_known_answers():
    for counter, key, want in KNOWN_ANSWERS:
        assert tuple(int(w) for w in RA.philox4x32_10(counter, key)) == want
    # vectorised over the counter as keep_mask uses it
    got = RA.philox4x32_10([np.array([0, 0x243F6A88]), np.array([0, 0x85A308D3]), np.array([0, 0x13198A2E]), np.array([0, 0x03707344])], (0, 0))
    assert [int(w[0]) for w in got] == list(KNOWN_ANSWERS[0][2])


def test_threshold_and_scale():
    assert RA.threshold(0.0) == 0 and RA.scale(0.0) == 1.0 and RA.keep_mask(5, 1, 3, 7, 0.0).all()
    assert RA.threshold(0.5) == 2 ** 31 and RA.p_eff(0.5) == 0.5 and RA.scale(0.5) == 2.0
    for p in (0.1, 0.25, 0.3, 0.9, 0.999):
        assert abs(RA.p_eff(p) - float(np.float32(p))) <= 2.0 ** -32 and abs(RA.p_eff(p) - p) <= 2.0 ** -16
    assert RA.scale(0.1).dtype == np.float32


def test_mask_is_a_function_of_its_five_values():
    """the same element from a larger batch, more queries and more keys: the same bit; word key & 3 of group key >> 2"""
    seed = RA.SEEDS["high"]
    big = RA.keep_mask(seed, 3, 21, 70, 0.5)
    assert np.array_equal(RA.keep_mask(seed, 1, 5, 9, 0.5), big[:1, :, :5, :9])
    words = RA.philox4x32_10((17, 20, 2 * 8 + 5, 0), (seed & 0xFFFFFFFF, seed >> 32))
    assert [bool(big[2, 5, 20, 68 + r]) for r in range(2)] == [int(words[r]) >= 2 ** 31 for r in range(2)]
    assert not np.array_equal(big, RA.keep_mask(seed ^ 1, 3, 21, 70, 0.5))


@pytest.mark.parametrize("name,p", [("tiny", 0.5), ("mid", 0.1), ("peaked", 0.1), ("block257", 0.5)])
def test_float64_statement_against_torch_autograd(name, p):
    args = RG.inputs(name)
    c = RG.CASES[name]
    z = RA.z_of(RA.keep_mask(RA.SEEDS["a"], c["B"], c["Kq"], c["N"], p), p)
    want = RA.torch_grads_masked(*args, z, torch.float64)
    for label, got, ref in zip(("out", "dq", "dk", "dv"), RA.attention_dropout_grad64(*args, z), want):
        err = RD.rel_err(got, ref)
        print(name, p, label, err)
        assert got.dtype == np.float64 and err < 1e-13, (label, err)      # two f64 evaluations in different orders
    plain = RG.attention_grad64(*args)
    for got, ref in zip(RA.attention_dropout_grad64(*args, np.ones_like(z)), plain):
        assert np.array_equal(got, ref)                                   # Z = 1: the statement without dropout


# ---- the mask as independent bits: conditions on the generator, each within 5 standard deviations --------------------------------

STAT_SHAPE = (2, 37, 437)


def _corr(a, b, r):
    """mean (a - r)(b - r) / (r (1 - r)) of two bit arrays and its standard deviation under independence, 1 / sqrt(pairs):
    E (a - r)^2 (b - r)^2 = (r (1 - r))^2, and products of overlapping pairs are uncorrelated"""
    return float(((a - r) * (b - r)).mean() / (r * (1 - r))), 1.0 / np.sqrt(a.size)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_statistics(p):
    B, Kq, N = STAT_SHAPE
    keep = RA.keep_mask(RA.SEEDS["a"], B, Kq, N, p).astype(np.float64)
    other = RA.keep_mask(RA.SEEDS["b"], B, Kq, N, p).astype(np.float64)
    r = 1.0 - RA.p_eff(p)
    sd = np.sqrt(r * (1 - r))
    checks = [("keep rate", keep.mean() - r, sd / np.sqrt(keep.size))]
    for b in range(B):
        for h in range(RD.NHEAD):
            checks.append((f"keep rate of plane {b}, {h}", keep[b, h].mean() - r, sd / np.sqrt(Kq * N)))
    checks.append(("lag 1 along keys", *_corr(keep[..., :-1], keep[..., 1:], r)))
    checks.append(("lag 1 along queries", *_corr(keep[:, :, :-1], keep[:, :, 1:], r)))
    checks.append(("adjacent heads", *_corr(keep[:, :-1], keep[:, 1:], r)))
    checks.append(("the two scenes", *_corr(keep[0], keep[1], r)))
    checks.append(("lag 4 along keys", *_corr(keep[..., :-4], keep[..., 4:], r)))
    agree = r * r + (1 - r) * (1 - r)
    checks.append(("agreement of two seeds one bit apart", (keep == other).mean() - agree, np.sqrt(agree * (1 - agree) / keep.size)))
    assert len(checks) == 23
    for label, deviation, sigma in checks:
        print(f"p = {p} {label}: {deviation / sigma:+.2f} sigma")
    for label, deviation, sigma in checks:
        assert abs(deviation) <= 5 * sigma, (label, deviation / sigma)


# ---- host-side decisions -----------------------------------------------------------------------------------------------------------


def test_argument_checks_of_the_dropout_arguments():
    q, k, v = torch.zeros(1, 5, 128), torch.zeros(1, 9, 128), torch.zeros(1, 9, 128)
    seed = torch.zeros(1, dtype=torch.int64)
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        for fn in (TD.attention_autograd, TD.attention_stats):
            with pytest.raises(AssertionError, match="dropout_p"):
                fn(q, k, v, dropout_p=bad, seed=seed)
        with pytest.raises(AssertionError):
            TD.attention_dropout_mask(seed, 1, 5, 9, bad)
    with pytest.raises(AssertionError, match="int64"):
        TD.attention_autograd(q, k, v, dropout_p=0.1, seed=seed.to(torch.int32))
    with pytest.raises(AssertionError, match="int64"):
        TD.attention_autograd(q, k, v, dropout_p=0.1, seed=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(AssertionError, match="int64"):
        TD.attention_stats(q, k, v, dropout_p=0.1, seed=None)
    with pytest.raises(AssertionError, match="int64"):
        TD.attention_autograd(q, k, v, dropout_p=0.1, seed=12345)
    with pytest.raises(AssertionError, match="on the device"):                 # dtype and size right, but a host tensor
        TD.attention_autograd(q, k, v, dropout_p=0.1, seed=seed)
    with pytest.raises(AssertionError, match="on the device"):
        TD.attention_backward(q, k, v, q, torch.zeros(1, 8, 5, 2), q, dropout_p=0.1, seed=seed)
    with pytest.raises(AssertionError, match="on the device"):
        TD.attention_dropout_mask(seed, 1, 5, 9, 0.1)
    with pytest.raises(AssertionError):
        TD.attention_autograd(q.double(), k, v, dropout_p=0.1, seed=seed)      # the plain checks still come first


def test_draw_dropout_seed_follows_torch_manual_seed():
    torch.manual_seed(3)
    a = TD.draw_dropout_seed(torch.device("cpu"))
    b = TD.draw_dropout_seed(torch.device("cpu"))
    torch.manual_seed(3)
    assert a.dtype == torch.int64 and a.shape == (1,) and torch.equal(TD.draw_dropout_seed(torch.device("cpu")), a) and not torch.equal(a, b)


def test_fused_attention_dropout_on_the_host():
    dec = TransformerDecoderLayer(RD.D, RD.NHEAD, 16, 0.1, "relu", self_posembed=PositionEmbeddingLearned(2, RD.D),
                                  cross_posembed=PositionEmbeddingLearned(2, RD.D)).train()
    assert dec.fused_attention_dropout is False and TransformerDecoderLayer.fused_attention_dropout is False
    dec.fused_attention_dropout = True
    assert "fused_attention_dropout" not in dec.state_dict() and "fused_attention_dropout" not in dict(dec.named_parameters())
    assert "fused_attention_dropout" not in dict(dec.named_buffers())
    dec.fused_attention_dropout = False
    query, key, query_pos, bev_pos = (torch.from_numpy(a) for a in RD.layer_inputs("tiny"))
    args = (query, key, query_pos, bev_pos)
    assert dec.fused_grad_reasons(*args) == ["attention dropout", "not on the device"]
    dec.fused_attention_grad = True                                            # the first attribute alone: still reported
    assert dec.fused_grad_reasons(*args) == ["attention dropout", "not on the device"]
    dec.fused_attention_dropout = True
    assert dec.fused_grad_reasons(*args) == ["not on the device"]
    mask = torch.zeros((1, key.shape[2]), dtype=torch.bool)
    assert dec.fused_grad_reasons(*args, key_padding_mask=mask) == ["mask", "not on the device"]
    dec.multihead_attn.dropout = 1.0                                           # the kernels take 0 <= p < 1
    assert "attention dropout" in dec.fused_grad_reasons(*args)
    dec.multihead_attn.dropout = 0.1
    dec.eval()
    assert dec.fused_grad_reasons(*args) == ["not on the device"]
    # both attributes change nothing off the device: forward is forward_plain, in train() with torch's dropout
    dec.train()
    torch.manual_seed(4)
    want = dec.forward_plain(*args)
    torch.manual_seed(4)
    assert torch.equal(dec(*args), want)
