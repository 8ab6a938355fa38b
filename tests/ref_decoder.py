"""Yardstick of the decoder tests: the case tables, the seeded input and weight generators, a float64 numpy restatement of
TransformerDecoderLayer (transfusion_utils.py:29-101, eval) and SeparateHead_Transfusion (transfusion_head.py:20-54, eval),
and the attention geometry restated from the rule documented at fnp_tf_attention_geometry (include/fnp.h).

tests/golden/make_decoder_golden.py runs the REFERENCE's modules on these inputs in f32 and stores their outputs, a CRC of
every input and, per case and tensor, err = max |reference f32 - this restatement| / max |this restatement|: the reference's
own f32 error.  tests/test_decoder_ref.py holds the restatement to the fixture inside err; the device is held to the
restatement within TOL_FACTOR x err (a long f32 sum taken in another order is another draw from the same error distribution,
and its maximum over a tensor's 10^4..10^5 elements varies by a small factor).

Weights are drawn with non-trivial BatchNorm running statistics and LayerNorm / BatchNorm affine parameters."""
import os
import zlib

import numpy as np

f32 = np.float32
D, NHEAD = 128, 8
TOL_FACTOR = 4.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_golden.npz")

NUSC_HEADS = dict(center=2, height=1, dim=3, rot=2, vel=2, heatmap=10)
NUSC_HEADS_NOVEL = dict(center=2, height=1, dim=3, rot=2, heatmap=10)

# (B, K, H, W), the FFN width, the heads (with and without vel), a bias in front of the heads' BatchNorm or not
LAYER_CASES = {
    "tiny": dict(B=1, K=5, H=3, W=3, F=16, heads=NUSC_HEADS_NOVEL, bias=False, seed=21),
    "mid": dict(B=2, K=37, H=23, W=19, F=256, heads=NUSC_HEADS, bias=True, seed=22),
    "mid16": dict(B=2, K=37, H=23, W=19, F=16, heads=NUSC_HEADS_NOVEL, bias=True, seed=23),
    "full": dict(B=2, K=200, H=180, W=180, F=256, heads=NUSC_HEADS, bias=False, seed=24),
}
# attention alone: (B, Kq, N)
ATT_CASES = {
    "att_tiny": dict(B=1, Kq=5, N=9, seed=31),
    "att_mid": dict(B=2, Kq=37, N=437, seed=32),
    "att_full": dict(B=2, Kq=200, N=32400, seed=33),
}
# end to end: HeatmapProposals -> init_queries -> DecoderHead -> BoxDecoder against the reference's predict + get_bboxes
E2E = dict(B=2, C=10, H=24, W=24, K=50, F=256, heads=NUSC_HEADS, bias=False, seed=41)
E2E_POST = {"SCORE_THRESH": 0.45, "POST_CENTER_RANGE": [-50.0, -61.2, -10.0, 61.2, 61.2, 10.0]}
E2E_STRIDE, E2E_VOXEL, E2E_PCR = 8, [0.075, 0.075, 0.2], [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def attention_geometry(n):
    """(split_len, tile_len): tile_len = 64, split_len = max(256, 64 * ceil(ceil(n / 64) / 64))"""
    per = -(-n // 64)
    return max(256, 64 * -(-per // 64)), 64


def create_2d_grid(x_size, y_size):
    """TransFusionHead.create_2D_grid: (1, x_size * y_size, 2), cell centres, first coordinate slowest"""
    xs, ys = np.meshgrid(np.linspace(0, x_size - 1, x_size, dtype=f32), np.linspace(0, y_size - 1, y_size, dtype=f32), indexing="ij")
    return np.stack([xs + f32(0.5), ys + f32(0.5)], 0).reshape(1, 2, -1).transpose(0, 2, 1).copy()


# ---- generators --------------------------------------------------------------------------------------------------------------


def _bn(rng, prefix, n, sd):
    sd[prefix + "weight"] = rng.uniform(0.5, 1.5, n).astype(f32)
    sd[prefix + "bias"] = rng.normal(0, 0.1, n).astype(f32)
    sd[prefix + "running_mean"] = rng.normal(0, 0.2, n).astype(f32)
    sd[prefix + "running_var"] = rng.uniform(0.5, 1.5, n).astype(f32)
    sd[prefix + "num_batches_tracked"] = np.array(7, np.int64)


def decoder_weights(seed, ffn):
    """state_dict of a TransformerDecoderLayer(128, 8, ffn, self_posembed=PositionEmbeddingLearned(2, 128), cross_posembed=same)"""
    rng = np.random.default_rng(seed)
    sd = {}
    for a in ("self_attn", "multihead_attn"):
        sd[a + ".in_proj_weight"] = rng.normal(0, 0.09, (3 * D, D)).astype(f32)
        sd[a + ".in_proj_bias"] = rng.normal(0, 0.05, 3 * D).astype(f32)
        sd[a + ".out_proj.weight"] = rng.normal(0, 0.09, (D, D)).astype(f32)
        sd[a + ".out_proj.bias"] = rng.normal(0, 0.05, D).astype(f32)
    sd["linear1.weight"] = rng.normal(0, 0.09, (ffn, D)).astype(f32)
    sd["linear1.bias"] = rng.normal(0, 0.05, ffn).astype(f32)
    sd["linear2.weight"] = rng.normal(0, 1.0 / np.sqrt(ffn), (D, ffn)).astype(f32)
    sd["linear2.bias"] = rng.normal(0, 0.05, D).astype(f32)
    for n in ("norm1", "norm2", "norm3"):
        sd[n + ".weight"] = rng.uniform(0.5, 1.5, D).astype(f32)
        sd[n + ".bias"] = rng.normal(0, 0.1, D).astype(f32)
    for pe in ("self_posembed", "cross_posembed"):
        p = pe + ".position_embedding_head."
        sd[p + "0.weight"] = rng.normal(0, 0.01, (D, 2, 1)).astype(f32)
        sd[p + "0.bias"] = rng.normal(0, 0.05, D).astype(f32)
        _bn(rng, p + "1.", D, sd)
        sd[p + "3.weight"] = rng.normal(0, 0.09, (D, D, 1)).astype(f32)
        sd[p + "3.bias"] = rng.normal(0, 0.05, D).astype(f32)
    return sd


def head_weights(seed, heads, bias):
    """state_dict of SeparateHead_Transfusion(128, 64, 1, {name: out_channels, num_conv 2}, use_bias=bias)"""
    rng = np.random.default_rng(seed + 1000)
    sd = {}
    for name, n_out in heads.items():
        sd[f"{name}.0.0.weight"] = rng.normal(0, 0.09, (64, D, 1)).astype(f32)
        if bias:
            sd[f"{name}.0.0.bias"] = rng.normal(0, 0.05, 64).astype(f32)
        _bn(rng, f"{name}.0.1.", 64, sd)
        sd[f"{name}.1.weight"] = rng.normal(0, 0.12, (n_out, 64, 1)).astype(f32)
        sd[f"{name}.1.bias"] = rng.normal(0, 0.5, n_out).astype(f32)
    return sd


def sep_head_dict(heads):
    return {name: dict(out_channels=n, num_conv=2) for name, n in heads.items()}


def layer_inputs(name):
    """query_feat (B, 128, K), lidar_feat (B, 128, H*W), query_pos (B, K, 2), bev_pos (1, H*W, 2), both positions in xy"""
    c = LAYER_CASES[name]
    rng = np.random.default_rng(c["seed"] + 500)
    B, K, N = c["B"], c["K"], c["H"] * c["W"]
    query = rng.normal(0, 1, (B, D, K)).astype(f32)
    key = rng.normal(0, 1, (B, D, N)).astype(f32)
    bev_pos = create_2d_grid(c["W"], c["H"])[..., ::-1].copy()
    idx = np.stack([rng.permutation(N)[:K] if N >= K else rng.integers(0, N, K) for _ in range(B)])
    query_pos = bev_pos[0][idx]
    return query, key, query_pos.astype(f32), bev_pos.astype(f32)


def e2e_inputs():
    """heatmap logits (B, C, H, W), all distinct and far apart after the sigmoid; features (B, 128, H, W); the class encoding's
    weight (128, C, 1) and bias (128)"""
    c = E2E
    rng = np.random.default_rng(c["seed"] + 500)
    n = c["B"] * c["C"] * c["H"] * c["W"]
    logits = np.linspace(-6, 2, n)[rng.permutation(n)].astype(f32).reshape(c["B"], c["C"], c["H"], c["W"])
    feat = rng.normal(0, 1, (c["B"], D, c["H"], c["W"])).astype(f32)
    enc_w = rng.normal(0, 0.5, (D, c["C"], 1)).astype(f32)
    enc_b = rng.normal(0, 0.5, D).astype(f32)
    return logits, feat, enc_w, enc_b


def attention_inputs(name):
    c = ATT_CASES[name]
    rng = np.random.default_rng(c["seed"])
    q = rng.normal(0, 1, (c["B"], c["Kq"], D)).astype(f32)
    k = rng.normal(0, 1, (c["B"], c["N"], D)).astype(f32)
    v = rng.normal(0, 1, (c["B"], c["N"], D)).astype(f32)
    return q, k, v


# ---- the float64 restatement -------------------------------------------------------------------------------------------------


def _d(a):
    return np.asarray(a, np.float64)


def attention64(q, k, v):
    """q (B, Kq, 128), k and v (B, N, 128) -> (B, Kq, 128): eight heads of 16, softmax(0.25 q.k) v"""
    q, k, v = _d(q), _d(k), _d(v)
    out = np.empty_like(q)
    for b in range(q.shape[0]):
        for h in range(NHEAD):
            sl = slice(16 * h, 16 * h + 16)
            s = 0.25 * (q[b][:, sl] @ k[b][:, sl].T)
            s -= s.max(1, keepdims=True)
            p = np.exp(s)
            out[b][:, sl] = (p @ v[b][:, sl]) / p.sum(1, keepdims=True)
    return out


def batchnorm64(x, sd, prefix, eps=1e-5):
    """x (..., C) with the channels last"""
    return (x - _d(sd[prefix + "running_mean"])) / np.sqrt(_d(sd[prefix + "running_var"]) + eps) * _d(sd[prefix + "weight"]) + _d(sd[prefix + "bias"])


def posembed64(sd, prefix, pos):
    """pos (B, P, 2) -> (B, P, 128)"""
    p = prefix + ".position_embedding_head."
    y = _d(pos) @ _d(sd[p + "0.weight"])[:, :, 0].T + _d(sd[p + "0.bias"])
    y = np.maximum(batchnorm64(y, sd, p + "1."), 0)
    return y @ _d(sd[p + "3.weight"])[:, :, 0].T + _d(sd[p + "3.bias"])


def layernorm64(x, sd, prefix, eps=1e-5):
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    return (x - mean) / np.sqrt(var + eps) * _d(sd[prefix + ".weight"]) + _d(sd[prefix + ".bias"])


def mha64(sd, prefix, q_in, k_in, v_in):
    w, b = _d(sd[prefix + ".in_proj_weight"]), _d(sd[prefix + ".in_proj_bias"])
    q = q_in @ w[:D].T + b[:D]
    k = k_in @ w[D:2 * D].T + b[D:2 * D]
    v = v_in @ w[2 * D:].T + b[2 * D:]
    return attention64(q, k, v) @ _d(sd[prefix + ".out_proj.weight"]).T + _d(sd[prefix + ".out_proj.bias"])


def layer64(sd, query, key, query_pos, key_pos):
    """-> (B, 128, K) in f64"""
    x = _d(query).transpose(0, 2, 1)
    kx = _d(key).transpose(0, 2, 1)
    qpe = posembed64(sd, "self_posembed", query_pos)
    kpe = posembed64(sd, "cross_posembed", key_pos)
    xp = x + qpe
    x = layernorm64(x + mha64(sd, "self_attn", xp, xp, xp), sd, "norm1")
    kp = kx + kpe
    x = layernorm64(x + mha64(sd, "multihead_attn", x + qpe, kp, kp), sd, "norm2")
    hid = np.maximum(x @ _d(sd["linear1.weight"]).T + _d(sd["linear1.bias"]), 0)
    x = layernorm64(x + (hid @ _d(sd["linear2.weight"]).T + _d(sd["linear2.bias"])), sd, "norm3")
    return x.transpose(0, 2, 1)


def heads64(hsd, heads, x, query_pos):
    """x (B, 128, K) -> {name: (B, n_out, K)} with center offset by query_pos"""
    rows = _d(x).transpose(0, 2, 1)
    out = {}
    for name in heads:
        y = rows @ _d(hsd[f"{name}.0.0.weight"])[:, :, 0].T
        if f"{name}.0.0.bias" in hsd:
            y = y + _d(hsd[f"{name}.0.0.bias"])
        y = np.maximum(batchnorm64(y, hsd, f"{name}.0.1."), 0)
        y = y @ _d(hsd[f"{name}.1.weight"])[:, :, 0].T + _d(hsd[f"{name}.1.bias"])
        out[name] = y.transpose(0, 2, 1)
    out["center"] = out["center"] + _d(query_pos).transpose(0, 2, 1)
    return out


_cache = {}


def layer_case64(name):
    """the restatement of a layer case, computed once per process: {'query_feat': .., head names ..} in f64"""
    if name not in _cache:
        c = LAYER_CASES[name]
        query, key, query_pos, bev_pos = layer_inputs(name)
        x = layer64(decoder_weights(c["seed"], c["F"]), query, key, query_pos, bev_pos)
        out = heads64(head_weights(c["seed"], c["heads"], c["bias"]), c["heads"], x, query_pos)
        out["query_feat"] = x
        _cache[name] = out
    return _cache[name]


def attention_case64(name):
    if name not in _cache:
        _cache[name] = attention64(*attention_inputs(name))
    return _cache[name]


def rel_err(got, want64):
    """max |got - want| / max |want|"""
    return float(np.abs(_d(got) - want64).max() / np.abs(want64).max())
