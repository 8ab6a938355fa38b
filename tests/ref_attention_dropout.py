"""Yardstick of the attention-dropout tests, written from the text of the attention dropout block of include/fnp.h:

the mask     keep(seed, scene, head, query, key): Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) on the counter
             (key >> 2, query, scene * 8 + head, 0); output word key & 3 belongs to `key`; keep iff word >= T,
             T = (uint32)((double)p * 2^32) with p rounded to f32 first (the C argument is a float); p_eff = T / 2^32 and the
             scale 1 / (1 - p_eff) evaluated in double and rounded to f32 once.
the operator O = (P o Z) V, Z = keep * scale, per head, with its gradients in float64 (ref_attention_grad.attention_grad64 with Z):

    dV_j = sum_i P_ij Z_ij dO_i,  D_i = dO_i . O_i,  dS_ij = P_ij (Z_ij dP_ij - D_i),  dK, dQ from dS as without dropout

tests/test_attention_dropout_ref.py holds the Philox core to the published known-answer vectors and the float64 statement to
torch's float64 autograd of the same masked expression.  The device is held to both in tests/test_gpu_attention_dropout.py."""
import numpy as np

import ref_attention_grad as RG

D, NHEAD = RG.D, RG.NHEAD
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two -> four uint32 arrays (Salmon et al. 2011, ten rounds)"""
    c = [np.asarray(x, np.uint64) for x in counter]
    k0, k1 = (np.asarray(x, np.uint64) for x in key)
    for _ in range(10):
        a, b = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(b >> np.uint64(32)) ^ c[1] ^ k0, b & MASK32, (a >> np.uint64(32)) ^ c[3] ^ k1, a & MASK32]
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return [x.astype(np.uint32) for x in c]


def threshold(p):
    """T of include/fnp.h; p goes through f32 as it does through the C ABI"""
    return int(float(np.float32(p)) * 2.0 ** 32)


def p_eff(p):
    return threshold(p) / 2.0 ** 32


def scale(p):
    """1 / (1 - p_eff), evaluated in double and rounded to f32 once -> np.float32"""
    return np.float32(1.0 / (1.0 - p_eff(p)))


def keep_mask(seed, B, Kq, N, p):
    """-> bool (B, 8, Kq, N); seed: a Python int in [0, 2^64)"""
    assert 0 <= seed < 2 ** 64
    groups = (N + 3) // 4
    plane = (np.arange(B, dtype=np.uint64)[:, None] * np.uint64(8) + np.arange(NHEAD, dtype=np.uint64)[None, :])[:, :, None, None]
    query = np.arange(Kq, dtype=np.uint64)[None, None, :, None]
    group = np.arange(groups, dtype=np.uint64)[None, None, None, :]
    shape = (B, NHEAD, Kq, groups)
    counter = [np.broadcast_to(x, shape) for x in (group, query, plane, np.uint64(0))]
    words = philox4x32_10(counter, (seed & 0xFFFFFFFF, seed >> 32))
    interleaved = np.stack(words, axis=-1).reshape(B, NHEAD, Kq, 4 * groups)[..., :N]      # word r of group j: key 4 j + r
    return interleaved >= np.uint32(threshold(p)) if threshold(p) else np.ones((B, NHEAD, Kq, N), bool)


def z_of(keep, p):
    """Z = keep * scale as float64 (the scale is the f32 value of the contract)"""
    return keep.astype(np.float64) * float(scale(p))


def attention_dropout_grad64(q, k, v, d_out, z):
    """z (B, 8, Kq, N) -> out, dq, dk, dv in float64"""
    q, k, v, d_out, z = (np.asarray(a, np.float64) for a in (q, k, v, d_out, z))
    out, dq, dk, dv = np.empty_like(q), np.empty_like(q), np.empty_like(k), np.empty_like(v)
    for b in range(q.shape[0]):
        for h in range(NHEAD):
            sl = slice(16 * h, 16 * h + 16)
            qh, kh, vh, doh = q[b][:, sl], k[b][:, sl], v[b][:, sl], d_out[b][:, sl]
            s = 0.25 * (qh @ kh.T)
            m = s.max(1, keepdims=True)
            lse = m + np.log(np.exp(s - m).sum(1, keepdims=True))
            p = np.exp(s - lse)
            pz = p * z[b, h]
            o = pz @ vh
            dd = (doh * o).sum(1, keepdims=True)
            ds = p * (z[b, h] * (doh @ vh.T) - dd)
            out[b][:, sl] = o
            dv[b][:, sl] = pz.T @ doh
            dk[b][:, sl] = 0.25 * (ds.T @ qh)
            dq[b][:, sl] = 0.25 * (ds @ kh)
    return out, dq, dk, dv


def attention_torch_masked(q, k, v, z):
    """the masked expression as torch ops: softmax, times z (B, 8, Kq, N), times v; differentiable, any dtype and device"""
    import torch

    B, Kq, _ = q.shape
    N = k.shape[1]
    heads = lambda t, rows: t.reshape(B, rows, NHEAD, 16).transpose(1, 2)
    p = torch.softmax(0.25 * (heads(q, Kq) @ heads(k, N).transpose(2, 3)), dim=-1)
    return ((p * z) @ heads(v, N)).transpose(1, 2).reshape(B, Kq, D)


def torch_grads_masked(q, k, v, d_out, z, dtype):
    """torch's autograd of attention_torch_masked in `dtype` on the CPU -> (out, dq, dk, dv) as numpy arrays"""
    import torch

    ts = [torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_() for a in (q, k, v)]
    out = attention_torch_masked(*ts, torch.from_numpy(np.asarray(z)).to(dtype))
    out.backward(torch.from_numpy(np.asarray(d_out)).to(dtype))
    return tuple(t.detach().numpy() for t in (out, ts[0].grad, ts[1].grad, ts[2].grad))


SEEDS = {"a": 0x0123456789ABCDEF, "b": 0x0123456789ABCDEE, "high": 0xFEDCBA9876543210}     # a and b differ in one bit
_cache = {}


def case(name, p, seed=SEEDS["a"]):
    """a case of ref_attention_grad.CASES under the mask of (seed, p), computed once per process ->
    dict(args, keep, z, want = the float64 statement, ref32 = torch's f32 autograd of the masked expression)"""
    key = (name, p, seed)
    if key not in _cache:
        import torch

        args = RG.inputs(name)
        c = RG.CASES[name]
        keep = keep_mask(seed, c["B"], c["Kq"], c["N"], p)
        z = z_of(keep, p)
        _cache[key] = dict(args=args, keep=keep, z=z, want=attention_dropout_grad64(*args, z),
                           ref32=torch_grads_masked(*args, z, torch.float32))
    return _cache[key]
