"""The yardstick of the attention-gradient tests held to torch's float64 autograd of the same expression, and what
attention_autograd and TransformerDecoderLayer.fused_grad_reasons decide on the host (no GPU)."""
import numpy as np
import pytest
import torch

import ref_attention_grad as RG
import ref_decoder as RD
from findnpropagate_amd.dense_heads import transfusion_decoder as TD
from findnpropagate_amd.model_utils.transfusion_utils import PositionEmbeddingLearned, TransformerDecoderLayer


@pytest.mark.parametrize("name", ["tiny", "mid", "peaked", "block257"])
def test_float64_statement_against_torch_autograd(name):
    args = RG.inputs(name)
    want = RG.torch_grads(*args, torch.float64)
    for label, got, ref in zip(("out", "dq", "dk", "dv"), RG.attention_grad64(*args), want):
        err = RD.rel_err(got, ref)
        print(name, label, err)
        assert got.dtype == np.float64 and err < 1e-13, (label, err)      # two f64 evaluations in different orders


def test_case_table():
    assert [(c["B"], c["Kq"], c["N"]) for c in RG.CASES.values()][:6] == \
        [(1, 5, 9), (2, 37, 437), (2, 300, 773), (1, 200, 16450), (1, 200, 32400), (2, 37, 437)]
    assert RG.CASES["peaked"]["scale"] == 6.0
    assert RD.attention_geometry(16450)[0] == 320 and RD.attention_geometry(16384)[0] == 256
    kb, wk = RG.BACKWARD_GEOMETRY
    assert {c["N"] for c in RG.CASES.values()} >= {wk, wk + 1, kb, kb + 1}
    q, k, v, d_out = RG.inputs("peaked")
    assert q.dtype == np.float32 and d_out.shape == q.shape and abs(float(q.std()) - 6.0) < 0.1


def test_argument_checks_of_attention_autograd():
    q, k, v = torch.zeros(1, 5, 128), torch.zeros(1, 9, 128), torch.zeros(1, 9, 128)
    with pytest.raises(AssertionError):
        TD.attention_autograd(q.double(), k, v)
    with pytest.raises(AssertionError):
        TD.attention_autograd(q, k, v[:, :8])
    with pytest.raises(AssertionError):
        TD.attention_autograd(q[0], k, v)
    with pytest.raises(AssertionError):
        TD.attention_autograd(torch.zeros(1, 2049, 128), k, v)
    with pytest.raises(AssertionError):
        TD.attention_autograd(q, k[:, :0], v[:, :0])
    with pytest.raises(AssertionError):
        TD.attention_autograd(torch.zeros(2, 5, 128), k, v)


def test_fused_grad_reasons_on_the_host():
    dec = TransformerDecoderLayer(RD.D, RD.NHEAD, 16, 0.1, "relu", self_posembed=PositionEmbeddingLearned(2, RD.D),
                                  cross_posembed=PositionEmbeddingLearned(2, RD.D)).eval()
    assert dec.fused_attention_grad is False and "fused_attention_grad" not in dec.state_dict()
    assert "fused_attention_grad" not in dict(dec.named_parameters())
    query, key, query_pos, bev_pos = (torch.from_numpy(a) for a in RD.layer_inputs("tiny"))
    assert dec.fused_grad_reasons(query, key, query_pos, bev_pos) == ["not on the device"]
    mask = torch.zeros((1, key.shape[2]), dtype=torch.bool)
    assert dec.fused_grad_reasons(query, key, query_pos, bev_pos, key_padding_mask=mask) == ["mask", "not on the device"]
    dec.train()
    assert "attention dropout" in dec.fused_grad_reasons(query, key, query_pos, bev_pos)
    assert "dtype" in dec.fused_grad_reasons(query.double(), key, query_pos, bev_pos)
    small = TransformerDecoderLayer(64, 4, 16, 0.0).train()
    r = small.fused_grad_reasons(torch.zeros(1, 64, 5), torch.zeros(1, 64, 9), torch.zeros(1, 5, 2), torch.zeros(1, 9, 2))
    assert "d_model / nhead" in r and "attention dropout" not in r
    # the flag changes nothing off the device: forward is forward_plain
    dec.eval()
    dec.fused_attention_grad = True
    q2 = query.clone().requires_grad_()
    with torch.no_grad():
        plain = dec.forward_plain(query, key, query_pos, bev_pos)
    assert torch.equal(dec(q2, key, query_pos, bev_pos).detach(), plain)
