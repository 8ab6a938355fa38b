"""attention_autograd (fnp_tf_attention_stats forward, csrc/tfattn_grad.hip backward) and the decoder layer's opt-in
fused_attention_grad route on the device: against the float64 statement of tests/ref_attention_grad.py within TOL_FACTOR = 4 x
the error of torch's own f32 autograd of the same expression on the same inputs (computed here, on the CPU), against an exact
one-hot construction, against themselves (bits from run to run, alone and in a batch, attention()'s bits in the forward), the
autograd plumbing, the derived memory bound and the layer's route selection.

Measured on one MI355X (error / yardstick error; allowed 4): out, dq, dk, dv over the ten cases 0.50-2.15 (largest: dq at N = 64,
2.15, and at N = 256, 2.14; N = 32,400 0.94-1.36; the peaked case 0.97-1.10); the layer in eval 0.72-1.55 over the output, the two
input gradients and the 30 parameter gradients, in train() with dropout 0 0.79-1.39; peak rise 6.3 MiB fused against 928.1 MiB for
the torch expression, one score tensor being 197.8 MiB."""
import copy

import numpy as np
import pytest
import torch

import ref_attention_grad as RG
import ref_decoder as RD
from findnpropagate_amd.dense_heads import transfusion_decoder as TD
from findnpropagate_amd.model_utils.transfusion_utils import PositionEmbeddingLearned, TransformerDecoderLayer

pytestmark = pytest.mark.gpu
NAMES = ("out", "dq", "dk", "dv")


def bits(t):
    return t.contiguous().view(torch.int32)


def dev_inputs(name, dev):
    return tuple(torch.from_numpy(a).to(dev) for a in RG.inputs(name))


def device_grads(q, k, v, d_out):
    """attention_autograd forward and backward -> out, dq, dk, dv (device tensors)"""
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    out = TD.attention_autograd(q, k, v)
    out.backward(d_out)
    return out.detach(), q.grad, k.grad, v.grad


# ---- 1. against f64, the tolerance from torch's f32 autograd ----------------------------------------------------------------


def test_backward_geometry_is_the_documented_one(cuda):
    for n in (1, 64, 257, 32400):
        assert TD.attention_backward_geometry(n) == RG.BACKWARD_GEOMETRY


@pytest.mark.parametrize("name", list(RG.CASES))
def test_gradients_against_float64(cuda, name):
    args = RG.inputs(name)
    want = RG.case64(name)
    ref32 = RG.torch_grads(*args, torch.float32)
    got = device_grads(*(torch.from_numpy(a).to(cuda) for a in args))
    worst = 0.0
    for label, g, r, w in zip(NAMES, got, ref32, want):
        assert g.shape == w.shape and g.is_contiguous()
        err = RD.rel_err(r, w)
        ratio = RD.rel_err(g.cpu().numpy(), w) / err
        print(f"attention grad {name} {label}: torch f32 error {err:.3e}, device error / that = {ratio:.3f}")
        assert 1e-8 < err < 1e-5, (label, err)
        worst = max(worst, ratio)
    assert worst <= RD.TOL_FACTOR


# ---- 2. one-hot attention: exact gradients -----------------------------------------------------------------------------------


def border_keys(n):
    split_len, tile_len = TD.attention_geometry(n)
    key_block, wave_keys = TD.attention_backward_geometry(n)
    keys = {0, n - 1}
    for step in (split_len, tile_len, key_block, wave_keys, 16):
        for edge in range(step, n, step):
            keys |= {edge - 1, edge}
    return sorted(keys)


@pytest.mark.parametrize("B,Kq,N", [(1, 5, 7), (2, 37, 437), (2, 37, 773)])
def test_one_hot_attention_has_exact_gradients(cuda, B, Kq, N):
    rng = np.random.default_rng(N)
    special = border_keys(N) if N > 16 else list(range(N))
    q = np.zeros((B, Kq, RD.D), np.float32)
    k = np.zeros((B, N, RD.D), np.float32)
    v = rng.integers(-4, 5, (B, N, RD.D)).astype(np.float32)
    d_out = rng.integers(-4, 5, (B, Kq, RD.D)).astype(np.float32)
    chosen = np.zeros((B, Kq, RD.NHEAD), np.int64)
    used = set()
    for b in range(B):
        for h in range(RD.NHEAD):
            mine = list(dict.fromkeys(special[(16 * h + 5 * b + j) % len(special)] for j in range(min(16, len(special)))))
            for d, n in enumerate(mine):
                k[b, n, 16 * h + d] = 16.0
            for j in range(Kq):
                d = (j + h) % len(mine)
                q[b, j, 16 * h + d] = 32.0                         # 0.25 * 32 * 16 = 128 against 0: exp(-128) is 0 in f32
                chosen[b, j, h] = mine[d]
                used.add(mine[d])
    if Kq >= 16:
        assert len(special) <= 16 * RD.NHEAD and set(special) <= used, "every border key is some query's chosen key"
    want_out, want_dv = np.empty_like(q), np.zeros_like(v)
    for b in range(B):
        for j in range(Kq):
            for h in range(RD.NHEAD):
                sl = slice(16 * h, 16 * h + 16)
                want_out[b, j, sl] = v[b, chosen[b, j, h], sl]
                want_dv[b, chosen[b, j, h], sl] += d_out[b, j, sl]      # at most Kq small integers: exact
    tq, tk, tv, tdo = (torch.from_numpy(a).to(cuda) for a in (q, k, v, d_out))
    out, stats = TD.attention_stats(tq, tk, tv)
    assert np.array_equal(out.cpu().numpy().view(np.int32), want_out.view(np.int32))
    assert torch.equal(stats[..., 0], torch.full_like(stats[..., 0], 128.0)) and torch.equal(stats[..., 1], torch.ones_like(stats[..., 1]))
    dq, dk, dv = (torch.full_like(t, float("nan")) for t in (tq, tk, tv))
    TD.attention_backward(tq, tk, tv, out, stats, tdo, dq, dk, dv)
    assert not bits(dq).any() and not bits(dk).any(), "P one-hot and dP - D = 0: every dS is +0"
    assert np.array_equal(dv.cpu().numpy().view(np.int32), want_dv.view(np.int32))


# ---- 3. bits -----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["tiny", "mid", "chunks", "block257"])
def test_forward_has_the_bits_of_attention(cuda, name):
    q, k, v, _ = dev_inputs(name, cuda)
    out = TD.attention_autograd(q.requires_grad_(), k, v)
    assert out.requires_grad and torch.equal(bits(out.detach()), bits(TD.attention(q, k, v)))


def test_backward_bits_run_to_run_and_batch_independence(cuda):
    rng = np.random.default_rng(7)
    q, k, v, d_out = (torch.from_numpy(rng.normal(0, 1, s).astype(np.float32)).to(cuda)
                      for s in ((3, 37, 128), (3, 437, 128), (3, 437, 128), (3, 37, 128)))
    whole = device_grads(q, k, v, d_out)
    again = device_grads(q, k, v, d_out)
    for label, a, b_ in zip(NAMES, whole, again):
        assert torch.equal(bits(a), bits(b_)), label
    for b in range(3):
        alone = device_grads(q[b:b + 1], k[b:b + 1], v[b:b + 1], d_out[b:b + 1])
        for label, a, w in zip(NAMES, alone, whole):
            assert torch.equal(bits(a[0]), bits(w[b])), (label, b)


# ---- 4. autograd plumbing ----------------------------------------------------------------------------------------------------


def test_only_the_gradients_asked_for(cuda):
    q, k, v, d_out = dev_inputs("mid", cuda)
    full = device_grads(q, k, v, d_out)
    v2 = v.clone().requires_grad_()
    q2 = q.clone()
    TD.attention_autograd(q2, k, v2).backward(d_out)
    assert q2.grad is None and torch.equal(bits(v2.grad), bits(full[3]))
    out, stats = TD.attention_stats(q, k, v)
    for want in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0)):       # NaN-filled buffers: an unwritten row shows
        bufs = [torch.full_like(t, float("nan")) if w else None for t, w in zip((q, k, v), want)]
        TD.attention_backward(q, k, v, out, stats, d_out, *bufs)
        for buf, ref in zip(bufs, full[1:]):
            assert buf is None or torch.equal(bits(buf), bits(ref)), want


def test_non_contiguous_grad_output_and_double_backward(cuda):
    q, k, v, d_out = dev_inputs("mid", cuda)
    full = device_grads(q, k, v, d_out)
    strided = torch.empty((d_out.shape[0], d_out.shape[1], 256), device=cuda)[..., ::2]
    strided.copy_(d_out)
    assert not strided.is_contiguous()
    for a, b_ in zip(device_grads(q, k, v, strided), full):
        assert torch.equal(bits(a), bits(b_))
    # through an op whose backward hands over an expanded (stride 0) gradient
    q3 = q.clone().requires_grad_()
    TD.attention_autograd(q3, k, v).sum().backward()
    assert torch.equal(bits(q3.grad), bits(device_grads(q, k, v, torch.ones_like(d_out))[1]))
    q4 = q.clone().requires_grad_()
    out = TD.attention_autograd(q4, k, v)
    (g,) = torch.autograd.grad(out, q4, d_out, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


# ---- 5. memory: no score tensor -----------------------------------------------------------------------------------------------


def peak_rise(fn, q, k, v, d_out):
    """the rise of max_memory_allocated over forward + backward of fn, above the inputs, out and the three gradients"""
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn(q, k, v)
    out.backward(d_out)
    torch.cuda.synchronize()
    results = sum(t.numel() * 4 for t in (out, q.grad, k.grad, v.grad))
    return torch.cuda.max_memory_allocated() - base - results


def test_no_tensor_of_score_size(cuda):
    args = dev_inputs("full", cuda)
    scores = 8 * 200 * 32400 * 4
    fused = peak_rise(TD.attention_autograd, *args)
    plain = peak_rise(RG.attention_torch, *args)
    print(f"peak rise over forward + backward: fused {fused / 2 ** 20:.1f} MiB, torch {plain / 2 ** 20:.1f} MiB, one score tensor {scores / 2 ** 20:.1f} MiB")
    assert fused < scores < plain


# ---- 6. the layer's route ----------------------------------------------------------------------------------------------------


def build(dev, dropout=0.1):
    c = RD.LAYER_CASES["mid"]
    dec = TransformerDecoderLayer(RD.D, RD.NHEAD, c["F"], dropout, "relu", self_posembed=PositionEmbeddingLearned(2, RD.D),
                                  cross_posembed=PositionEmbeddingLearned(2, RD.D))
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in RD.decoder_weights(c["seed"], c["F"]).items()}, strict=True)
    return dec.eval().to(dev)


def layer_grads(dec, route, args):
    """loss = out.square().sum() through `route` -> {'out', 'query', 'key', parameter names}: numpy arrays"""
    dec.zero_grad(set_to_none=True)
    query, key = (t.detach().clone().requires_grad_() for t in args[:2])
    out = route(query, key, *args[2:])
    out.square().sum().backward()
    res = {"out": out.detach(), "query": query.grad, "key": key.grad}
    res.update({n: p.grad for n, p in dec.named_parameters()})
    assert all(t is not None for t in res.values())
    return {n: t.cpu().numpy() for n, t in res.items()}


# In train() the BatchNorm behind a position embedding's first convolution subtracts the batch mean, so that convolution's bias
# has a gradient of zero by construction: the float64 copy returns ~1e-16, both f32 routes return rounding noise, and an error
# relative to max |truth| means nothing.  Those two tensors are left out in train(); in eval (running statistics) they are held.
ZERO_BY_CONSTRUCTION_IN_TRAIN = ("self_posembed.position_embedding_head.0.bias", "cross_posembed.position_embedding_head.0.bias")


def held_to_truth(dec, args, label, leave_out=()):
    """the fused route's output and gradients within TOL_FACTOR x forward_plain's own f32 error against a float64 copy"""
    truth_dec = copy.deepcopy(dec).double()
    truth = layer_grads(truth_dec, truth_dec.forward_plain, tuple(t.double() for t in args))
    plain = layer_grads(dec, dec.forward_plain, args)
    dec.fused_attention_grad = True
    assert dec.fused_grad_reasons(*args) == []
    fused = layer_grads(dec, dec, args)
    worst = 0.0
    assert set(leave_out) <= set(truth)
    for n in truth:
        if n in leave_out:
            assert np.abs(truth[n]).max() < 1e-9 * np.abs(truth["query"]).max(), n       # zero indeed
            continue
        err = RD.rel_err(plain[n], truth[n])
        ratio = RD.rel_err(fused[n], truth[n]) / err
        print(f"layer {label} {n}: forward_plain f32 error {err:.3e}, fused route error / that = {ratio:.3f}")
        worst = max(worst, ratio)
    assert worst <= RD.TOL_FACTOR
    return plain, fused


def layer_inputs(dev):
    query, key, query_pos, bev_pos = (torch.from_numpy(a).to(dev) for a in RD.layer_inputs("mid"))
    return query, key, query_pos, bev_pos.repeat(2, 1, 1)


def test_layer_gradients_on_the_fused_route(cuda):
    dec = build(cuda)
    plain, fused = held_to_truth(dec, layer_inputs(cuda), "eval")
    assert not np.array_equal(plain["out"], fused["out"]), "the two routes are different code"


def test_layer_route_selection(cuda):
    """which route forward takes.  The forward's bits name it (forward_plain and the fused route differ in bits, as
    test_layer_gradients_on_the_fused_route asserts).  Gradients are not compared by bits: two runs of forward_plain itself
    differ in the weight gradients of cross_posembed's convolutions on an MI355X (torch's Conv1d weight gradient over the key
    positions is not reproducible from run to run; the test prints which tensors differ).  Wherever forward_plain is due,
    forward_fused_grad must not be called at all."""
    dec = build(cuda)
    args = layer_inputs(cuda)

    def no_fused(*a, **kw):
        raise AssertionError("forward_fused_grad was called")

    dec.forward_fused_grad = no_fused
    plain = layer_grads(dec, dec.forward_plain, args)
    again = layer_grads(dec, dec.forward_plain, args)
    print("forward_plain twice, tensors whose bits differ:", [n for n in plain if not np.array_equal(plain[n].view(np.int32), again[n].view(np.int32))])
    off = layer_grads(dec, dec, args)                                   # flag off: forward_plain
    assert np.array_equal(off["out"].view(np.int32), plain["out"].view(np.int32))
    dec.fused_attention_grad = True
    mask = torch.zeros((2, args[1].shape[2]), dtype=torch.bool, device=cuda)
    want = layer_grads(dec, lambda *a: dec.forward_plain(*a, key_padding_mask=mask), args)
    got = layer_grads(dec, lambda *a: dec(*a, key_padding_mask=mask), args)
    assert np.array_equal(got["out"].view(np.int32), want["out"].view(np.int32))
    with torch.no_grad():                                              # no reason against the eval device path: it runs
        dec.requires_grad_(False)
        assert dec.plain_reasons(*args) == []
        dec.fused_attention_grad = False
        eval_out = dec(*args)
        dec.fused_attention_grad = True
        assert torch.equal(dec(*args), eval_out)
        dec.requires_grad_(True)
    dec.train()                                                         # dropout 0.1: attention dropout is active
    assert "attention dropout" in dec.fused_grad_reasons(*args)
    torch.manual_seed(11)
    a = dec(*args)
    torch.manual_seed(11)
    assert torch.equal(a, dec.forward_plain(*args))


def test_layer_in_train_mode_without_dropout_takes_the_fused_route(cuda):
    dec = build(cuda, dropout=0.0).train()
    plain, fused = held_to_truth(dec, layer_inputs(cuda), "train, dropout 0", ZERO_BY_CONSTRUCTION_IN_TRAIN)
    assert not np.array_equal(plain["out"], fused["out"])
