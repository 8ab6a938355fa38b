"""Yardstick of the attention-gradient tests: the case table, the seeded generators and a float64 numpy statement of the
attention core out = softmax(0.25 q.k^T) v per head with its gradients, written from the formulas of the
fnp_tf_attention_backward block of include/fnp.h:

    P_ij = exp(s_ij - lse_i), D_i = sum_d dO_id O_id, dP_ij = dO_i . v_j, dS_ij = P_ij (dP_ij - D_i)
    dV_j = sum_i P_ij dO_i,   dK_j = 0.25 sum_i dS_ij q_i,   dQ_i = 0.25 sum_j dS_ij k_j

tests/test_attention_grad_ref.py holds it to torch's float64 autograd of the same expression.  The device is held to it within
ref_decoder.TOL_FACTOR x the error of torch's own f32 autograd on the same inputs (tests/test_gpu_attention_grad.py)."""
import numpy as np

import ref_decoder as RD

f32 = np.float32
D, NHEAD = RD.D, RD.NHEAD

# (B, Kq, N); scale multiplies q (6: a peaked softmax)
CASES = {
    "tiny": dict(B=1, Kq=5, N=9, seed=51, scale=1.0),
    "mid": dict(B=2, Kq=37, N=437, seed=52, scale=1.0),                 # two splits, a ragged last tile, Kq no multiple of 16
    "chunks": dict(B=2, Kq=300, N=773, seed=53, scale=1.0),             # three splits, Kq crosses the 256-query chunk
    "split320": dict(B=1, Kq=200, N=16450, seed=54, scale=1.0),         # the smallest class with split_len above 256 (320)
    "full": dict(B=1, Kq=200, N=32400, seed=55, scale=1.0),
    "peaked": dict(B=2, Kq=37, N=437, seed=56, scale=6.0),
    # the backward's own geometry (key_block = 256 keys per workgroup, wave_keys = 64 per wave): each side of each border
    "wave64": dict(B=1, Kq=17, N=64, seed=57, scale=1.0),
    "wave65": dict(B=1, Kq=17, N=65, seed=58, scale=1.0),
    "block256": dict(B=1, Kq=17, N=256, seed=59, scale=1.0),
    "block257": dict(B=1, Kq=17, N=257, seed=60, scale=1.0),
}
BACKWARD_GEOMETRY = (256, 64)      # (key_block, wave_keys): constants (include/fnp.h)


def inputs(name):
    """q (B, Kq, 128), k, v (B, N, 128), d_out (B, Kq, 128): N(0, 1) in f32, q times the case's scale"""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    q = (rng.normal(0, 1, (c["B"], c["Kq"], D)) * c["scale"]).astype(f32)
    k = rng.normal(0, 1, (c["B"], c["N"], D)).astype(f32)
    v = rng.normal(0, 1, (c["B"], c["N"], D)).astype(f32)
    d_out = rng.normal(0, 1, (c["B"], c["Kq"], D)).astype(f32)
    return q, k, v, d_out


def attention_grad64(q, k, v, d_out):
    """-> out, dq, dk, dv in float64"""
    q, k, v, d_out = (np.asarray(a, np.float64) for a in (q, k, v, d_out))
    out, dq, dk, dv = np.empty_like(q), np.empty_like(q), np.empty_like(k), np.empty_like(v)
    for b in range(q.shape[0]):
        for h in range(NHEAD):
            sl = slice(16 * h, 16 * h + 16)
            qh, kh, vh, doh = q[b][:, sl], k[b][:, sl], v[b][:, sl], d_out[b][:, sl]
            s = 0.25 * (qh @ kh.T)
            m = s.max(1, keepdims=True)
            lse = m + np.log(np.exp(s - m).sum(1, keepdims=True))
            p = np.exp(s - lse)
            o = p @ vh
            dd = (doh * o).sum(1, keepdims=True)
            ds = p * (doh @ vh.T - dd)
            out[b][:, sl] = o
            dv[b][:, sl] = p.T @ doh
            dk[b][:, sl] = 0.25 * (ds.T @ qh)
            dq[b][:, sl] = 0.25 * (ds @ kh)
    return out, dq, dk, dv


def attention_torch(q, k, v):
    """the same expression as torch ops (the core of nn.MultiheadAttention): differentiable, any dtype and device"""
    import torch

    B, Kq, _ = q.shape
    N = k.shape[1]
    heads = lambda t, rows: t.reshape(B, rows, NHEAD, 16).transpose(1, 2)
    p = torch.softmax(0.25 * (heads(q, Kq) @ heads(k, N).transpose(2, 3)), dim=-1)
    return (p @ heads(v, N)).transpose(1, 2).reshape(B, Kq, D)


def torch_grads(q, k, v, d_out, dtype, device="cpu"):
    """torch's autograd of attention_torch in `dtype` -> (out, dq, dk, dv) as numpy arrays"""
    import torch

    ts = [torch.from_numpy(np.asarray(a)).to(device=device, dtype=dtype).requires_grad_() for a in (q, k, v)]
    out = attention_torch(*ts)
    out.backward(torch.from_numpy(np.asarray(d_out)).to(device=device, dtype=dtype))
    return tuple(t.detach().cpu().numpy() for t in (out, ts[0].grad, ts[1].grad, ts[2].grad))


_cache = {}


def case64(name):
    """attention_grad64 of a case, computed once per process"""
    if name not in _cache:
        _cache[name] = attention_grad64(*inputs(name))
    return _cache[name]
