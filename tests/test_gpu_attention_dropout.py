"""Attention dropout inside the fused forward and backward (the fnp_tf_attention_dropout_* block of include/fnp.h) on the device:
the mask against the numpy restatement of tests/ref_attention_dropout.py exactly; out, dq, dk, dv against its float64 statement
within TOL_FACTOR = 4 x the error of torch's own f32 autograd of the same masked expression on the same inputs (computed here,
on the CPU); an exact one-hot construction at p = 0.5; bits (run to run, the statistics, p = 0, scene 0 alone and in a batch);
the autograd plumbing (the seed is saved with the forward); the derived memory bound; the layer's fused_attention_dropout route.

Measured on one MI355X (error / yardstick error; allowed 4): out, dq, dk, dv over the nine cases at p = 0.1 0.45-3.57 (largest: out of
`mid`, 3.57, where the yardstick's own error is at its smallest, 1.4e-7; all others below 2.0), `mid` at p = 0.5 1.84-2.93; the layer in
train() 0.74-1.23 over the output, the two input gradients and 28 parameter gradients; peak rise 6.4 MiB, one score tensor being
197.8 MiB."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_attention_dropout as RA
import ref_attention_grad as RG
import ref_decoder as RD
from findnpropagate_amd import lib
from findnpropagate_amd.dense_heads import transfusion_decoder as TD
from test_gpu_attention_grad import ZERO_BY_CONSTRUCTION_IN_TRAIN, bits, border_keys, build, layer_grads, layer_inputs, peak_rise

pytestmark = pytest.mark.gpu
NAMES = ("out", "dq", "dk", "dv")
SEED = RA.SEEDS["a"]


def seed_tensor(seed, dev):
    """a Python int in [0, 2^64) as the int64 device tensor the library reads as a uint64"""
    return torch.tensor([seed - 2 ** 64 if seed >= 2 ** 63 else seed], dtype=torch.int64, device=dev)


def device_grads(q, k, v, d_out, p, seed):
    """attention_autograd with dropout, forward and backward -> out, dq, dk, dv (device tensors)"""
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    out = TD.attention_autograd(q, k, v, p, seed)
    out.backward(d_out)
    return out.detach(), q.grad, k.grad, v.grad


def random_inputs(dev, B, Kq, N, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return tuple(torch.randn(s, generator=g, device=dev) for s in ((B, Kq, RD.D), (B, N, RD.D), (B, N, RD.D), (B, Kq, RD.D)))


# ---- 1. the mask, exactly ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("name", ["tiny", "mid", "chunks", "wave65", "block257"])
def test_device_mask_is_the_numpy_mask(cuda, name, p):
    c = RG.CASES[name]
    for seed in (SEED, RA.SEEDS["high"]):                              # the second one has the sign bit of the int64 set
        got = TD.attention_dropout_mask(seed_tensor(seed, cuda), c["B"], c["Kq"], c["N"], p)
        assert got.dtype == torch.bool and got.shape == (c["B"], RD.NHEAD, c["Kq"], c["N"])
        assert np.array_equal(got.cpu().numpy(), RA.keep_mask(seed, c["B"], c["Kq"], c["N"], p)), hex(seed)


# ---- 2. against f64, the tolerance from torch's f32 autograd of the masked expression ---------------------------------------------


@pytest.mark.parametrize("name,p", [(n, 0.1) for n in RG.CASES if n != "full"] + [("mid", 0.5)])
def test_gradients_against_float64(cuda, name, p):
    ref = RA.case(name, p)
    got = device_grads(*(torch.from_numpy(a).to(cuda) for a in ref["args"]), p, seed_tensor(SEED, cuda))
    worst = 0.0
    for label, g, r, w in zip(NAMES, got, ref["ref32"], ref["want"]):
        assert g.shape == w.shape and g.is_contiguous()
        err = RD.rel_err(r, w)
        ratio = RD.rel_err(g.cpu().numpy(), w) / err
        print(f"attention dropout grad {name} p = {p} {label}: torch f32 error {err:.3e}, device error / that = {ratio:.3f}")
        assert 1e-8 < err < 1e-5, (label, err)
        worst = max(worst, ratio)
    assert worst <= RD.TOL_FACTOR


# ---- 3. one-hot attention at p = 0.5: exact ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("B,Kq,N", [(1, 5, 7), (2, 37, 437), (2, 37, 773)])
def test_one_hot_attention_with_dropout_is_exact(cuda, B, Kq, N):
    """the construction of test_one_hot_attention_has_exact_gradients: every query's softmax is one-hot on a chosen key (many of
    them on the borders of splits, tiles, key blocks and waves).  At p = 0.5 the scale is 2: out is 2 v[chosen] or 0, dv the
    scatter-add of 2 dO over the kept pairs (small integers, exact in any order), dS = 0 everywhere."""
    rng = np.random.default_rng(N)
    special = border_keys(N) if N > 16 else list(range(N))
    q = np.zeros((B, Kq, RD.D), np.float32)
    k = np.zeros((B, N, RD.D), np.float32)
    v = rng.integers(-4, 5, (B, N, RD.D)).astype(np.float32)
    d_out = rng.integers(-4, 5, (B, Kq, RD.D)).astype(np.float32)
    chosen = np.zeros((B, Kq, RD.NHEAD), np.int64)
    for b in range(B):
        for h in range(RD.NHEAD):
            mine = list(dict.fromkeys(special[(16 * h + 5 * b + j) % len(special)] for j in range(min(16, len(special)))))
            for d, n in enumerate(mine):
                k[b, n, 16 * h + d] = 16.0
            for j in range(Kq):
                d = (j + h) % len(mine)
                q[b, j, 16 * h + d] = 32.0                         # 0.25 * 32 * 16 = 128 against 0: exp(-128) is 0 in f32
                chosen[b, j, h] = mine[d]
    keep = RA.keep_mask(SEED, B, Kq, N, 0.5)
    want_out, want_dv = np.zeros_like(q), np.zeros_like(v)
    kept = 0
    for b in range(B):
        for j in range(Kq):
            for h in range(RD.NHEAD):
                sl = slice(16 * h, 16 * h + 16)
                if keep[b, h, j, chosen[b, j, h]]:
                    want_out[b, j, sl] = 2.0 * v[b, chosen[b, j, h], sl]
                    want_dv[b, chosen[b, j, h], sl] += 2.0 * d_out[b, j, sl]
                    kept += 1
    assert 0 < kept < B * Kq * RD.NHEAD, "both kept and dropped pairs occur"
    tq, tk, tv, tdo = (torch.from_numpy(a).to(cuda) for a in (q, k, v, d_out))
    seed = seed_tensor(SEED, cuda)
    out, stats = TD.attention_stats(tq, tk, tv, dropout_p=0.5, seed=seed)
    assert np.array_equal(out.cpu().numpy().view(np.int32), want_out.view(np.int32))
    assert torch.equal(stats[..., 0], torch.full_like(stats[..., 0], 128.0)) and torch.equal(stats[..., 1], torch.ones_like(stats[..., 1]))
    dq, dk, dv = (torch.full_like(t, float("nan")) for t in (tq, tk, tv))
    TD.attention_backward(tq, tk, tv, out, stats, tdo, dq, dk, dv, dropout_p=0.5, seed=seed)
    assert not bits(dq).any() and not bits(dk).any(), "P one-hot and Z dP - D = 0 on the chosen key: every dS is a zero"
    assert np.array_equal(dv.cpu().numpy().view(np.int32), want_dv.view(np.int32))


# ---- 4. bits ---------------------------------------------------------------------------------------------------------------------------


def test_same_seed_same_bits_and_another_seed_another_output(cuda):
    q, k, v, d_out = random_inputs(cuda, 2, 37, 437, 1)
    one = device_grads(q, k, v, d_out, 0.1, seed_tensor(SEED, cuda))
    two = device_grads(q, k, v, d_out, 0.1, seed_tensor(SEED, cuda))
    for label, a, b_ in zip(NAMES, one, two):
        assert torch.equal(bits(a), bits(b_)), label
    other = device_grads(q, k, v, d_out, 0.1, seed_tensor(RA.SEEDS["b"], cuda))
    assert not torch.equal(bits(other[0]), bits(one[0]))
    assert not torch.equal(bits(one[0]), bits(TD.attention(q, k, v)))


@pytest.mark.parametrize("name", ["tiny", "mid", "chunks", "block257"])
def test_statistics_do_not_see_the_mask(cuda, name):
    q, k, v, _ = (torch.from_numpy(a).to(cuda) for a in RG.inputs(name))
    _, plain = TD.attention_stats(q, k, v)
    _, dropped = TD.attention_stats(q, k, v, dropout_p=0.5, seed=seed_tensor(SEED, cuda))
    assert torch.equal(bits(plain), bits(dropped))


@pytest.mark.parametrize("name", ["tiny", "mid", "chunks", "block257"])
def test_p_zero_through_the_dropout_entry_points_has_the_plain_bits(cuda, name):
    """attention_stats and attention_backward run the plain calls at dropout_p == 0, so the dropout entry points are called here"""
    q, k, v, d_out = (torch.from_numpy(a).to(cuda) for a in RG.inputs(name))
    B, Kq, N = TD.check_attention(q, k, v)
    L = lib.load()
    seed = seed_tensor(SEED, cuda)
    want_out, want_stats = TD.attention_stats(q, k, v)
    assert torch.equal(bits(want_out), bits(TD.attention(q, k, v)))
    want = [torch.empty_like(t) for t in (q, k, v)]
    TD.attention_backward(q, k, v, want_out, want_stats, d_out, *want)
    out, stats = torch.full_like(want_out, float("nan")), torch.full_like(want_stats, float("nan"))
    ws_bytes = L.fnp_tf_attention_workspace_bytes(B, Kq, N)
    ws = torch.empty(max(ws_bytes // 4, 4), dtype=torch.float32, device=cuda)
    lib.check(L.fnp_tf_attention_dropout_stats(lib.ptr(q), lib.ptr(k), lib.ptr(v), B, Kq, N, lib.ptr(ws), ws_bytes, lib.ptr(out),
                                               lib.ptr(stats), 0.0, lib.ptr(seed), lib.stream()), "fnp_tf_attention_dropout_stats")
    assert torch.equal(bits(out), bits(want_out)) and torch.equal(bits(stats), bits(want_stats))
    got = [torch.full_like(t, float("nan")) for t in (q, k, v)]
    ws_bytes = L.fnp_tf_attention_backward_workspace_bytes(B, Kq, N)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=cuda)
    lib.check(L.fnp_tf_attention_dropout_backward(lib.ptr(q), lib.ptr(k), lib.ptr(v), lib.ptr(out), lib.ptr(stats), lib.ptr(d_out), B, Kq, N,
                                                  lib.ptr(ws), ws_bytes, *(lib.ptr(t) for t in got), 0.0, lib.ptr(seed), lib.stream()),
              "fnp_tf_attention_dropout_backward")
    for label, a, b_ in zip(NAMES[1:], got, want):
        assert torch.equal(bits(a), bits(b_)), label
    for bad in (-0.5, 1.0, float("nan")):                              # 0 <= p < 1, or nothing is launched
        assert L.fnp_tf_attention_dropout_stats(lib.ptr(q), lib.ptr(k), lib.ptr(v), B, Kq, N, lib.ptr(ws), ws_bytes, lib.ptr(out),
                                                lib.ptr(stats), bad, lib.ptr(seed), lib.stream()) < 0


def test_scene_zero_alone_and_in_a_batch(cuda):
    """the scene index is part of the counter: a batch and its first scene alone agree, the other scenes have other masks"""
    q, k, v, d_out = random_inputs(cuda, 3, 37, 437, 2)
    seed = seed_tensor(SEED, cuda)
    whole = device_grads(q, k, v, d_out, 0.1, seed)
    alone = device_grads(q[:1], k[:1], v[:1], d_out[:1], 0.1, seed)
    for label, a, w in zip(NAMES, alone, whole):
        assert torch.equal(bits(a[0]), bits(w[0])), label
    second = device_grads(q[1:2], k[1:2], v[1:2], d_out[1:2], 0.1, seed)
    assert not torch.equal(bits(second[0][0]), bits(whole[0][1]))


# ---- 5. autograd plumbing ------------------------------------------------------------------------------------------------------------


def test_only_the_gradients_asked_for(cuda):
    q, k, v, d_out = (torch.from_numpy(a).to(cuda) for a in RG.inputs("mid"))
    seed = seed_tensor(SEED, cuda)
    full = device_grads(q, k, v, d_out, 0.1, seed)
    v2 = v.clone().requires_grad_()
    q2 = q.clone()
    TD.attention_autograd(q2, k, v2, 0.1, seed).backward(d_out)
    assert q2.grad is None and torch.equal(bits(v2.grad), bits(full[3]))
    out, stats = TD.attention_stats(q, k, v, dropout_p=0.1, seed=seed)
    assert torch.equal(bits(out), bits(full[0]))
    for want in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0)):       # NaN-filled buffers: an unwritten row shows
        bufs = [torch.full_like(t, float("nan")) if w else None for t, w in zip((q, k, v), want)]
        TD.attention_backward(q, k, v, out, stats, d_out, *bufs, dropout_p=0.1, seed=seed)
        for buf, ref in zip(bufs, full[1:]):
            assert buf is None or torch.equal(bits(buf), bits(ref)), want


def test_the_backward_uses_the_seed_of_the_forward(cuda):
    q, k, v, d_out = (torch.from_numpy(a).to(cuda) for a in RG.inputs("mid"))
    torch.manual_seed(5)
    want = device_grads(q, k, v, d_out, 0.1, TD.draw_dropout_seed(cuda))
    torch.manual_seed(5)
    q1, k1, v1 = (t.clone().requires_grad_() for t in (q, k, v))
    out = TD.attention_autograd(q1, k1, v1, 0.1)                       # no seed given: drawn from torch's generator
    torch.manual_seed(99)                                              # the generator moves on; the saved seed does not
    torch.rand(3, device=cuda)
    out.backward(d_out)
    for label, a, b_ in zip(NAMES, (out.detach(), q1.grad, k1.grad, v1.grad), want):
        assert torch.equal(bits(a), bits(b_)), label
    given = seed_tensor(SEED, cuda)                                    # a caller's seed tensor overwritten after the forward
    want = device_grads(q, k, v, d_out, 0.1, seed_tensor(SEED, cuda))
    q2 = q.clone().requires_grad_()
    out = TD.attention_autograd(q2, k, v, 0.1, given)
    given.fill_(7)
    out.backward(d_out)
    assert torch.equal(bits(q2.grad), bits(want[1]))


def test_manual_seed_reproduces_the_forward(cuda):
    q, k, v, _ = (torch.from_numpy(a).to(cuda) for a in RG.inputs("mid"))
    torch.manual_seed(21)
    a = TD.attention_autograd(q, k, v, 0.1)
    b_ = TD.attention_autograd(q, k, v, 0.1)
    torch.manual_seed(21)
    assert torch.equal(bits(TD.attention_autograd(q, k, v, 0.1)), bits(a)) and not torch.equal(bits(a), bits(b_))
    s = TD.draw_dropout_seed(cuda)
    assert s.dtype == torch.int64 and s.shape == (1,) and s.device == q.device


# ---- 6. memory: no score tensor, no mask -----------------------------------------------------------------------------------------------


def test_no_tensor_of_score_size(cuda):
    args = random_inputs(cuda, 1, 200, 32400, 3)
    seed = seed_tensor(SEED, cuda)
    scores = 8 * 200 * 32400 * 4
    fused = peak_rise(lambda q, k, v: TD.attention_autograd(q, k, v, 0.1, seed), *args)
    print(f"peak rise over forward + backward with dropout: fused {fused / 2 ** 20:.1f} MiB, one score tensor {scores / 2 ** 20:.1f} MiB")
    assert fused < scores


# ---- 7. the layer ------------------------------------------------------------------------------------------------------------------------


def cross_masked(dec, keep, scale):
    """nn.MultiheadAttention(q_in, m, m)[0] of dec.multihead_attn as torch ops with the explicit masked expression in its core"""
    def cross(q_in, m, key_padding_mask, attn_mask):
        mha = dec.multihead_attn
        w, b, d = mha.in_proj_weight, mha.in_proj_bias, mha.embed_dim
        rows_q, rows_m = q_in.transpose(0, 1), m.transpose(0, 1)
        q = F.linear(rows_q, w[:d], b[:d])
        k = F.linear(rows_m, w[d:2 * d], b[d:2 * d])
        v = F.linear(rows_m, w[2 * d:], b[2 * d:])
        z = keep.to(q.dtype) * scale
        return F.linear(RA.attention_torch_masked(q, k, v, z), mha.out_proj.weight, mha.out_proj.bias).transpose(0, 1)
    return cross


def train_layer_with_only_the_cross_attention_mask(dev):
    dec = build(dev, dropout=0.1).train()
    for m in (dec.dropout, dec.dropout1, dec.dropout2, dec.dropout3):
        m.p = 0.0
    dec.self_attn.dropout = 0.0
    assert dec.multihead_attn.dropout == 0.1
    return dec


def test_layer_with_fused_attention_dropout(cuda, monkeypatch):
    dec = train_layer_with_only_the_cross_attention_mask(cuda)
    args = layer_inputs(cuda)
    seed = seed_tensor(SEED, cuda)
    monkeypatch.setattr(TD, "draw_dropout_seed", lambda device: seed)
    keep = TD.attention_dropout_mask(seed, 2, 37, 437, 0.1)
    assert np.array_equal(keep.cpu().numpy(), RA.keep_mask(SEED, 2, 37, 437, 0.1))
    scale = float(RA.scale(0.1))
    truth_dec = copy.deepcopy(dec).double()
    truth = layer_grads(truth_dec, lambda *a: truth_dec._forward_torch(*a, None, None, cross_masked(truth_dec, keep, scale)),
                        tuple(t.double() for t in args))
    plain = layer_grads(dec, lambda *a: dec._forward_torch(*a, None, None, cross_masked(dec, keep, scale)), args)
    dec.fused_attention_grad = True
    assert "attention dropout" in dec.fused_grad_reasons(*args)
    dec.fused_attention_dropout = True
    assert dec.fused_grad_reasons(*args) == []
    fused = layer_grads(dec, dec, args)
    assert len([n for n, _ in dec.named_parameters()]) == 30
    worst = 0.0
    for n in truth:
        if n in ZERO_BY_CONSTRUCTION_IN_TRAIN:
            assert np.abs(truth[n]).max() < 1e-9 * np.abs(truth["query"]).max(), n       # zero indeed
            continue
        err = RD.rel_err(plain[n], truth[n])
        ratio = RD.rel_err(fused[n], truth[n]) / err
        print(f"layer train, attention dropout 0.1 {n}: torch f32 error {err:.3e}, fused route error / that = {ratio:.3f}")
        worst = max(worst, ratio)
    assert worst <= RD.TOL_FACTOR


def test_layer_route_with_and_without_the_attribute(cuda, monkeypatch):
    dec = train_layer_with_only_the_cross_attention_mask(cuda)
    args = layer_inputs(cuda)
    dec.fused_attention_grad = True

    def no_fused(*a, **kw):
        raise AssertionError("forward_fused_grad was called")

    fused_route = dec.forward_fused_grad
    dec.forward_fused_grad = no_fused                                   # attribute off: forward_plain with torch's dropout
    assert dec.fused_attention_dropout is False and "attention dropout" in dec.fused_grad_reasons(*args)
    torch.manual_seed(11)
    a = dec(*args)
    torch.manual_seed(11)
    assert torch.equal(a, dec.forward_plain(*args))
    dec.forward_fused_grad = fused_route
    dec.eval()                                                          # eval: no dropout, today's fused route bit for bit
    assert dec.fused_grad_reasons(*args) == []
    today = dec(*args)
    dec.fused_attention_dropout = True
    monkeypatch.setattr(TD, "draw_dropout_seed", no_fused)              # and no seed is drawn
    assert dec.fused_grad_reasons(*args) == []
    assert torch.equal(bits(dec(*args).detach()), bits(today.detach()))
    assert not torch.equal(bits(today.detach()), bits(dec.forward_plain(*args).detach())), "the fused route, not forward_plain"
