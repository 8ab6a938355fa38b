"""TransFusionHead's decoder layer and prediction heads on the device (transfusion_head.py:315-319 of predict): the
reference's TransformerDecoderLayer (one nn.MultiheadAttention of 200 queries over the 180 x 180 BEV cells, a self-attention,
two position-embedding MLPs, three LayerNorms, the FFN) and SeparateHead_Transfusion (six Conv1d + BatchNorm1d + ReLU + Conv1d
heads) are several dozen launches per scene in torch, with 8 x 200 x 32 400 scores written out and read back; here they are
seven launches of csrc/tfdecoder.hip (eight with more than 256 queries) on one stream, with nothing read on the host.

SeparateHead_Transfusion keeps the reference's names and init.  attention(q, k, v) is the attention kernel alone;
attention_autograd(q, k, v) is the same forward (bit for bit) with a backward on csrc/tfattn_grad.hip, which the decoder layer's
opt-in fused_attention_grad route uses for its cross attention under autograd.  With dropout_p > 0 it applies dropout to the
probabilities inside the kernels, by a counter-based mask of a device-side seed that the backward regenerates (include/fnp.h;
the layer's fused_attention_dropout).
DecoderHead(decoder, prediction_head)(query_feat, lidar_feat_flatten, query_pos, bev_pos) returns the reference's res_layer
dict with `center` already offset.  Both DecoderHead and TransformerDecoderLayer.forward fall back to the modules called
plainly whenever decoder_plain_reasons() / heads_plain_reasons() find something against the device path.

The packed parameters (BatchNorm folded from the running statistics) and cross_posembed(bev_pos), which in eval depend on
weights and on bev_pos only, are computed once with torch ops and cached; the cache key is (data_ptr, _version) of EVERY
parameter and buffer slot of the modules, slots holding None included, and (data_ptr, _version, shape) of bev_pos, so an
in-place update, load_state_dict or a slot filled later all invalidate it.  The cache keeps bev_pos alive, so its address
cannot be handed to another tensor while the key is held."""
import ctypes

import torch
from torch import nn

from .. import lib

D_MODEL, N_HEAD, HEAD_MID, MAX_HEADS, MAX_QUERIES = 128, 8, 64, 8, 2048


class SeparateHead_Transfusion(nn.Module):
    """One small Conv1d stack per entry of sep_head_dict ({name: {'out_channels': n, 'num_conv': c}}), registered under the
    entry's name: c - 1 blocks of Conv1d(input_channels -> head_channels, bias=use_bias) + BatchNorm1d + ReLU, then a
    Conv1d(head_channels -> n) with bias; a head whose name contains 'hm' starts with its last bias at init_bias.  Modules are
    created head by head, front to back, so a seeded construction draws what the reference draws and its checkpoints load
    with strict=True.  forward(x (B, input_channels, P)) -> {name: (B, n, P)}."""

    def __init__(self, input_channels, head_channels, kernel_size, sep_head_dict, init_bias=-2.19, use_bias=False):
        super().__init__()
        self.sep_head_dict = sep_head_dict
        pad = kernel_size // 2
        for name, spec in sep_head_dict.items():
            stack = [nn.Sequential(nn.Conv1d(input_channels, head_channels, kernel_size, padding=pad, bias=use_bias),
                                   nn.BatchNorm1d(head_channels), nn.ReLU()) for _ in range(spec["num_conv"] - 1)]
            last = nn.Conv1d(head_channels, spec["out_channels"], kernel_size, padding=pad, bias=True)
            if "hm" in name:
                nn.init.constant_(last.bias, init_bias)
            self.add_module(name, nn.Sequential(*stack, last))

    def forward(self, x):
        return {name: getattr(self, name)(x) for name in self.sep_head_dict}


# ---- attention alone -------------------------------------------------------------------------------------------------------


def attention_geometry(n_keys):
    """(split_len, tile_len) of fnp_tf_attention for n_keys keys: a function of n_keys alone"""
    L = lib.load()
    s, t = ctypes.c_int(), ctypes.c_int()
    lib.check(L.fnp_tf_attention_geometry(int(n_keys), ctypes.byref(s), ctypes.byref(t)), "fnp_tf_attention_geometry")
    return s.value, t.value


def check_attention(q, k, v):
    """host-side argument checks of attention (no library needed) -> B, Kq, N"""
    for name, t in (("q", q), ("k", k), ("v", v)):
        assert isinstance(t, torch.Tensor) and t.dim() == 3 and t.shape[2] == D_MODEL, f"{name}: (B, rows, {D_MODEL})"
        assert t.dtype == torch.float32, f"{name} must be float32, got {t.dtype}"
    B, Kq, N = int(q.shape[0]), int(q.shape[1]), int(k.shape[1])
    assert k.shape == v.shape and k.shape[0] == B, "k and v: (B, N, 128) with q's B"
    assert 1 <= Kq <= MAX_QUERIES, f"1 <= Kq <= {MAX_QUERIES}"
    assert 1 <= N < 2 ** 31 // D_MODEL, "1 <= N < 2^31 / 128"
    return B, Kq, N


def attention(q, k, v, out=None):
    """q (B, Kq, 128), k and v (B, N, 128) f32 on the device -> (B, Kq, 128): eight heads of 16 columns, softmax(0.25 q.k) v,
    before any output projection.  Bit-identical from run to run and for a scene alone or inside a batch.  No gradient."""
    B, Kq, N = check_attention(q, k, v)
    L = lib.load()
    lib.require_device(q, k, v)
    q, k, v = q.detach().contiguous(), k.detach().contiguous(), v.detach().contiguous()
    if out is None:
        out = torch.empty((B, Kq, D_MODEL), dtype=torch.float32, device=q.device)
    assert out.shape == (B, Kq, D_MODEL) and out.dtype == torch.float32 and out.is_contiguous()
    if B == 0:
        return out
    ws_bytes = L.fnp_tf_attention_workspace_bytes(B, Kq, N)
    if ws_bytes < 0:
        raise lib.FnpError(f"fnp_tf_attention_workspace_bytes({B}, {Kq}, {N}) failed")
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=q.device) if ws_bytes else None
    lib.check(L.fnp_tf_attention(lib.ptr(q), lib.ptr(k), lib.ptr(v), B, Kq, N, lib.ptr(ws), ws_bytes, lib.ptr(out), lib.stream()),
              "fnp_tf_attention")
    return out


def attention_backward_geometry(n_keys):
    """(key_block, wave_keys) of fnp_tf_attention_backward's key-stationary kernel: constants, 256 and 64"""
    L = lib.load()
    kb, wk = ctypes.c_int(), ctypes.c_int()
    lib.check(L.fnp_tf_attention_backward_geometry(int(n_keys), ctypes.byref(kb), ctypes.byref(wk)), "fnp_tf_attention_backward_geometry")
    return kb.value, wk.value


def _workspace(L, fn, B, Kq, N, dev):
    ws_bytes = getattr(L, fn)(B, Kq, N)
    if ws_bytes < 0:
        raise lib.FnpError(f"{fn}({B}, {Kq}, {N}) failed")
    return (torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev) if ws_bytes else None), ws_bytes


def check_dropout(dropout_p, seed, device=None):
    """host-side argument checks of the dropout arguments (no library needed, nothing read from the seed) -> p as a float"""
    p = float(dropout_p)
    assert 0.0 <= p < 1.0, f"0 <= dropout_p < 1, got {dropout_p}"
    if p > 0.0:
        assert isinstance(seed, torch.Tensor) and seed.dtype == torch.int64 and seed.numel() == 1, "seed: one int64 on the device"
        assert seed.is_cuda and (device is None or seed.device == device), "seed: on the device of q, k and v"
    return p


def draw_dropout_seed(device):
    """one int64 drawn on `device` from torch's generator for that device (torch.manual_seed reproduces it): the seed of one
    attention dropout mask.  No host read."""
    return torch.empty(1, dtype=torch.int64, device=device).random_()


def attention_dropout_mask(seed, B, Kq, N, p):
    """keep(seed, scene, head, query, key) of include/fnp.h as a bool tensor (B, 8, Kq, N), written by the device function the
    kernels call.  For tests and tools: no training path calls it."""
    assert 0 <= B and 1 <= Kq <= MAX_QUERIES and 1 <= N < 2 ** 31 // D_MODEL
    assert isinstance(seed, torch.Tensor) and seed.dtype == torch.int64 and seed.numel() == 1 and seed.is_cuda, "seed: one int64 on the device"
    assert 0.0 <= float(p) < 1.0, f"0 <= p < 1, got {p}"
    L = lib.load()
    keep = torch.empty((B, N_HEAD, Kq, N), dtype=torch.uint8, device=seed.device)
    lib.check(L.fnp_tf_attention_dropout_mask(lib.ptr(seed), float(p), B, Kq, N, lib.ptr(keep), lib.stream()), "fnp_tf_attention_dropout_mask")
    return keep.bool()


def attention_stats(q, k, v, out=None, stats=None, dropout_p=0.0, seed=None):
    """attention() that also returns the softmax statistics: -> out (B, Kq, 128), stats (B, 8, Kq, 2) holding (M, L) per scene,
    head and query (include/fnp.h).  out has attention()'s bits.  No gradient; attention_autograd is the differentiable form.
    With dropout_p > 0 and seed (one int64 on the device) out is the dropped output (P o Z) V; stats do not see the mask."""
    B, Kq, N = check_attention(q, k, v)
    p = check_dropout(dropout_p, seed, q.device)
    L = lib.load()
    lib.require_device(q, k, v)
    q, k, v = q.detach().contiguous(), k.detach().contiguous(), v.detach().contiguous()
    if out is None:
        out = torch.empty((B, Kq, D_MODEL), dtype=torch.float32, device=q.device)
    if stats is None:
        stats = torch.empty((B, N_HEAD, Kq, 2), dtype=torch.float32, device=q.device)
    assert out.shape == (B, Kq, D_MODEL) and out.dtype == torch.float32 and out.is_contiguous()
    assert stats.shape == (B, N_HEAD, Kq, 2) and stats.dtype == torch.float32 and stats.is_contiguous()
    if B:
        ws, ws_bytes = _workspace(L, "fnp_tf_attention_workspace_bytes", B, Kq, N, q.device)
        if p == 0.0:
            lib.check(L.fnp_tf_attention_stats(lib.ptr(q), lib.ptr(k), lib.ptr(v), B, Kq, N, lib.ptr(ws), ws_bytes, lib.ptr(out),
                                               lib.ptr(stats), lib.stream()), "fnp_tf_attention_stats")
        else:
            lib.check(L.fnp_tf_attention_dropout_stats(lib.ptr(q), lib.ptr(k), lib.ptr(v), B, Kq, N, lib.ptr(ws), ws_bytes, lib.ptr(out),
                                                       lib.ptr(stats), p, lib.ptr(seed), lib.stream()), "fnp_tf_attention_dropout_stats")
    return out, stats


def attention_backward(q, k, v, out, stats, d_out, dq=None, dk=None, dv=None, dropout_p=0.0, seed=None):
    """fnp_tf_attention_backward on contiguous f32 device tensors: writes the gradients into whichever of dq (B, Kq, 128), dk
    and dv (B, N, 128) are given and skips the others; out and stats as attention_stats returned them, with the same dropout_p
    and seed (then fnp_tf_attention_dropout_backward regenerates the forward's mask)"""
    B, Kq, N = check_attention(q, k, v)
    p = check_dropout(dropout_p, seed, q.device)
    L = lib.load()
    lib.require_device(q, k, v, out, stats, d_out, dq, dk, dv)
    assert out.shape == q.shape and d_out.shape == q.shape and stats.shape == (B, N_HEAD, Kq, 2)
    for t, like in ((dq, q), (dk, k), (dv, v)):
        assert t is None or (t.shape == like.shape and t.dtype == torch.float32)
    assert all(t.dtype == torch.float32 for t in (out, stats, d_out))
    if B and (dq is not None or dk is not None or dv is not None):
        ws, ws_bytes = _workspace(L, "fnp_tf_attention_backward_workspace_bytes", B, Kq, N, q.device)
        if p == 0.0:
            lib.check(L.fnp_tf_attention_backward(lib.ptr(q), lib.ptr(k), lib.ptr(v), lib.ptr(out), lib.ptr(stats), lib.ptr(d_out), B, Kq, N,
                                                  lib.ptr(ws), ws_bytes, lib.ptr(dq), lib.ptr(dk), lib.ptr(dv), lib.stream()),
                      "fnp_tf_attention_backward")
        else:
            lib.check(L.fnp_tf_attention_dropout_backward(lib.ptr(q), lib.ptr(k), lib.ptr(v), lib.ptr(out), lib.ptr(stats), lib.ptr(d_out),
                                                          B, Kq, N, lib.ptr(ws), ws_bytes, lib.ptr(dq), lib.ptr(dk), lib.ptr(dv), p,
                                                          lib.ptr(seed), lib.stream()), "fnp_tf_attention_dropout_backward")
    return dq, dk, dv


class _AttentionGrad(torch.autograd.Function):
    """attention_stats forward, attention_backward (csrc/tfattn_grad.hip) backward.  Saved for the backward: q, k, v, out and
    the (M, L) statistics (B, 8, Kq, 2); nothing with Kq x N elements exists at any time.  With dropout the seed is saved too
    (a copy: the caller may overwrite its tensor), so the backward's mask is the forward's whatever the generator did since."""

    @staticmethod
    def forward(ctx, q, k, v, dropout_p, seed):
        q, k, v = q.detach().contiguous(), k.detach().contiguous(), v.detach().contiguous()
        ctx.dropout_p = dropout_p
        if dropout_p > 0.0:
            seed = seed.detach().clone()
            out, stats = attention_stats(q, k, v, dropout_p=dropout_p, seed=seed)
            ctx.save_for_backward(q, k, v, out, stats, seed)
        else:
            out, stats = attention_stats(q, k, v)
            ctx.save_for_backward(q, k, v, out, stats)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        q, k, v, out, stats, *seed = ctx.saved_tensors
        grads = [torch.empty_like(t) if need else None for t, need in zip((q, k, v), ctx.needs_input_grad)]
        if seed:
            attention_backward(q, k, v, out, stats, d_out.contiguous(), *grads, dropout_p=ctx.dropout_p, seed=seed[0])
        else:
            attention_backward(q, k, v, out, stats, d_out.contiguous(), *grads)
        return (*grads, None, None)


def attention_autograd(q, k, v, dropout_p=0.0, seed=None):
    """attention(q, k, v) under autograd: the same values bit for bit, and gradients for whichever of q, k, v require them
    (dq, dk, dv of softmax(0.25 q.k) v; the scores are recomputed tile by tile, never stored).  A second derivative raises.
    dropout_p > 0: dropout on the probabilities inside the kernels, the mask of include/fnp.h regenerated in the backward from
    `seed` (one int64 on the device; None draws one with draw_dropout_seed)."""
    check_attention(q, k, v)
    p = float(dropout_p)
    if p > 0.0 and seed is None:
        seed = draw_dropout_seed(q.device)
    p = check_dropout(p, seed, q.device)
    return _AttentionGrad.apply(q, k, v, p, seed if p > 0.0 else None)


# ---- path selection ----------------------------------------------------------------------------------------------------------


def _slots(*modules):
    """every parameter and buffer slot of the modules, those holding None included, in a fixed order"""
    out = []
    for root in modules:
        if root is None:
            continue
        for m in root.modules():
            for name in m._parameters:
                out.append((m._parameters, name))
            for name in m._buffers:
                out.append((m._buffers, name))
    return out


def cache_key(decoder, prediction_head, key_pos):
    """the key of the packed parameters and the cached key position embedding.  An address names a tensor only while its
    storage lives: DevicePack keeps an alias of every keyed storage (and key_pos itself) for as long as it holds the key, so
    no address in a held key can be handed to other data."""
    key = [None if d[n] is None else (d[n].data_ptr(), d[n]._version) for d, n in _slots(decoder, prediction_head)]
    key.append((key_pos.data_ptr(), key_pos._version, tuple(key_pos.shape), str(key_pos.device)))
    return tuple(key)


def _is_posembed(m):
    from ..model_utils.transfusion_utils import PositionEmbeddingLearned

    if not isinstance(m, PositionEmbeddingLearned):
        return False
    h = m.position_embedding_head
    if len(h) != 4 or not isinstance(h[1], nn.BatchNorm1d) or h[1].running_mean is None or h[1].running_var is None:
        return False                            # (no running statistics: eval normalises with the batch's, nothing to fold)
    return tuple(h[0].weight.shape) == (D_MODEL, 2, 1) and h[0].bias is not None and tuple(h[3].weight.shape) == (D_MODEL, D_MODEL, 1) \
        and h[3].bias is not None


def decoder_static_reasons(decoder):
    """what in the module itself (structure, parameter dtype and placement) stands against the device path"""
    r = []
    if decoder.cross_only:
        r.append("cross_only")
    if getattr(decoder, "activation_name", None) != "relu":
        r.append("activation")
    mha = decoder.multihead_attn
    if mha.embed_dim != D_MODEL or mha.num_heads != N_HEAD or mha.in_proj_weight is None or mha.in_proj_bias is None:
        r.append("d_model / nhead")
    ffn = decoder.linear1.out_features
    if ffn % 16 or not 16 <= ffn <= 1024:
        r.append("dim_feedforward")
    if not (_is_posembed(decoder.self_posembed) and _is_posembed(decoder.cross_posembed)):
        r.append("position embedding")
    return r + _placement_reasons(decoder)


def _placement_reasons(module):
    """parameters and floating-point buffers (the running statistics) alike: f32, on one device"""
    r = []
    tensors = list(module.parameters()) + [b for b in module.buffers() if b.is_floating_point()]
    if any(t.dtype != torch.float32 for t in tensors):
        r.append("dtype")
    if not all(t.is_cuda for t in tensors) or len({t.device for t in tensors}) > 1:
        r.append("not on the device")
    return r


def _any_training(*roots):
    return any(m.training for root in roots if root is not None for m in root.modules())


def dynamic_reasons(decoder, prediction_head, query, key, query_pos, key_pos, key_padding_mask=None, attn_mask=None):
    """what in this call (mode, masks, autograd on the inputs, their dtype, placement and shapes) stands against the device path"""
    r = []
    if _any_training(decoder, prediction_head):        # any submodule: a BatchNorm or Dropout left in train() alone counts
        r.append("training mode")
    if key_padding_mask is not None or attn_mask is not None:
        r.append("mask")
    tensors = (query, key, query_pos, key_pos)
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        r.append("autograd")
    if any(t.dtype != torch.float32 for t in tensors):
        r.append("dtype")
    if not all(t.is_cuda for t in tensors):
        r.append("not on the device")
    if not r:
        ok = query.dim() == 3 and key.dim() == 3 and query.shape[1] == D_MODEL and key.shape[:2] == (query.shape[0], D_MODEL)
        if ok:
            B, K, N = int(query.shape[0]), int(query.shape[2]), int(key.shape[2])
            ok = B >= 1 and 1 <= K <= MAX_QUERIES and 1 <= N < 2 ** 31 // D_MODEL and tuple(query_pos.shape) == (B, K, 2)
            ok = ok and key_pos.shape[-2:] == (N, 2) and (key_pos.dim() == 2 or (key_pos.dim() == 3 and key_pos.shape[0] in (1, B)))
        if not ok:
            r.append("shape")
    return r


def _merge(*lists):
    return list(dict.fromkeys(x for l in lists for x in l))


def decoder_plain_reasons(decoder, query, key, query_pos, key_pos, key_padding_mask=None, attn_mask=None):
    """what stands against the device path of the decoder layer (empty list: it runs on the device)"""
    r = dynamic_reasons(decoder, None, query, key, query_pos, key_pos, key_padding_mask, attn_mask)
    if torch.is_grad_enabled() and any(p.requires_grad for p in decoder.parameters()):
        r = _merge(r, ["autograd"])
    return _merge(r, decoder_static_reasons(decoder))


def _head_parts(fc):
    """(conv1, bn, conv2) of a two-convolution head with 1-wide kernels, or None"""
    if not isinstance(fc, nn.Sequential) or len(fc) != 2 or not isinstance(fc[0], nn.Sequential) or len(fc[0]) != 3:
        return None
    conv1, bn, act = fc[0]
    conv2 = fc[1]
    if not (isinstance(conv1, nn.Conv1d) and isinstance(bn, nn.BatchNorm1d) and isinstance(act, nn.ReLU) and isinstance(conv2, nn.Conv1d)):
        return None
    if conv1.kernel_size != (1,) or conv2.kernel_size != (1,) or bn.running_mean is None or bn.running_var is None:
        return None
    if tuple(conv1.weight.shape[:2]) != (HEAD_MID, D_MODEL) or conv2.weight.shape[1] != HEAD_MID or not 1 <= conv2.weight.shape[0] <= 64:
        return None
    return conv1, bn, conv2


def heads_static_reasons(prediction_head):
    r = []
    names = list(prediction_head.sep_head_dict)
    if not 1 <= len(names) <= MAX_HEADS:
        r.append("number of heads")
    if any(_head_parts(getattr(prediction_head, n)) is None for n in names):
        r.append("head layout (kernel_size, num_conv, channels)")
    elif "center" in names and getattr(prediction_head, "center")[1].weight.shape[0] != 2:
        r.append("center head")
    if "center" not in names:
        r.append("no center head")
    return r + _placement_reasons(prediction_head)


def heads_plain_reasons(prediction_head):
    """what stands against the device path of the prediction heads"""
    r = ["training mode"] if _any_training(prediction_head) else []
    if torch.is_grad_enabled() and any(p.requires_grad for p in prediction_head.parameters()):
        r.append("autograd")
    return _merge(r, heads_static_reasons(prediction_head))


# ---- packing -----------------------------------------------------------------------------------------------------------------


def _fold(conv_w, conv_b, bn):
    """Conv1d (1-wide) followed by an eval BatchNorm1d as one affine map: W' = W * s, b' = (b - mean) * s + beta"""
    s = torch.rsqrt(bn.running_var + bn.eps) if bn.weight is None else bn.weight / torch.sqrt(bn.running_var + bn.eps)
    w = conv_w.reshape(conv_w.shape[0], -1) * s[:, None]
    b = -bn.running_mean if conv_b is None else conv_b - bn.running_mean
    b = b * s
    if bn.bias is not None:
        b = b + bn.bias
    return w, b


def pack_params(decoder, prediction_head=None):
    """the packed parameter block of fnp_tf_decoder (include/fnp.h) -> params (f32, flat), head names, head_out, center_head"""
    with torch.no_grad():
        dev = decoder.linear1.weight.device
        pe = decoder.self_posembed.position_embedding_head
        w1, b1 = _fold(pe[0].weight, pe[0].bias, pe[1])
        parts = [torch.tensor([decoder.norm1.eps, decoder.norm2.eps, decoder.norm3.eps, 0.0], dtype=torch.float32, device=dev),
                 w1, b1, pe[3].weight, pe[3].bias]
        for mha, norm in ((decoder.self_attn, decoder.norm1), (decoder.multihead_attn, decoder.norm2)):
            parts += [mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias, norm.weight, norm.bias]
        parts += [decoder.linear1.weight, decoder.linear1.bias, decoder.linear2.weight, decoder.linear2.bias,
                  decoder.norm3.weight, decoder.norm3.bias]
        names, head_out, center = [], [], -1
        if prediction_head is not None:
            names = list(prediction_head.sep_head_dict)
            first_w, first_b, last_w, last_b = [], [], [], []
            for i, n in enumerate(names):
                conv1, bn, conv2 = _head_parts(getattr(prediction_head, n))
                w, b = _fold(conv1.weight, conv1.bias, bn)
                first_w.append(w), first_b.append(b)
                n_out = int(conv2.weight.shape[0])
                pad = (n_out + 15) // 16 * 16
                pw = torch.zeros((pad, HEAD_MID), dtype=torch.float32, device=dev)
                pb = torch.zeros((pad,), dtype=torch.float32, device=dev)
                pw[:n_out] = conv2.weight.reshape(n_out, HEAD_MID)
                pb[:n_out] = conv2.bias
                last_w.append(pw), last_b.append(pb)
                head_out.append(n_out)
                if n == "center":
                    center = i
            parts += first_w + first_b + last_w + last_b
        params = torch.cat([p.detach().reshape(-1).to(torch.float32) for p in parts]).contiguous()
    return params, names, head_out, center


class DevicePack:
    """the cached device-side state of one (decoder, prediction_head or None) pair and the call into fnp_tf_decoder"""

    def __init__(self, decoder, prediction_head):
        self.decoder, self.prediction_head = decoder, prediction_head
        self.key = None

    def reasons(self, query, key, query_pos, key_pos, key_padding_mask=None, attn_mask=None):
        """decoder_plain_reasons (+ heads_plain_reasons) at the cost of one cache key: what depends on the modules alone is
        kept with the key, and the parameters' requires_grad is looked at only while autograd records"""
        r = dynamic_reasons(self.decoder, self.prediction_head, query, key, query_pos, key_pos, key_padding_mask, attn_mask)
        if torch.is_grad_enabled():
            mods = [m for m in (self.decoder, self.prediction_head) if m is not None]
            if any(p.requires_grad for m in mods for p in m.parameters()):
                r = _merge(r, ["autograd"])
        if r:                                   # the plain span runs anyway: name everything that stands against the device path
            return _merge(r, self._static_reasons())
        self.refresh(key_pos)
        return self.static

    def _static_reasons(self):
        return decoder_static_reasons(self.decoder) + (heads_static_reasons(self.prediction_head) if self.prediction_head is not None else [])

    def refresh(self, key_pos):
        key = cache_key(self.decoder, self.prediction_head, key_pos)
        if key == self.key:
            return
        self.key = None
        self.static = self._static_reasons()
        if self.static:
            self.key_pos, self.key = key_pos, key
            self.held = [d[n].detach() for d, n in _slots(self.decoder, self.prediction_head) if d[n] is not None]
            return
        self.params, self.names, self.head_out, self.center = pack_params(self.decoder, self.prediction_head)
        with torch.no_grad():
            pos = key_pos if key_pos.dim() == 3 else key_pos[None]
            self.key_pe = self.decoder.cross_posembed(pos).contiguous()          # (1 or B, 128, N): channel-major, as the kernel reads it
        self.key_pos = key_pos                                                    # held: its address stays its own
        self.held = [d[n].detach() for d, n in _slots(self.decoder, self.prediction_head) if d[n] is not None]   # aliases: so do theirs
        self.head_out_c = (ctypes.c_int * max(1, len(self.head_out)))(*self.head_out)
        self.key = key

    def run(self, query, key, query_pos, key_pos):
        """-> query_feat (B, 128, K), {head name: (B, n_out, K)}"""
        L = lib.load()
        self.refresh(key_pos)
        assert not self.static, self.static
        B, _, K = (int(s) for s in query.shape)
        N = int(key.shape[2])
        dev = query.device
        query, key, query_pos = query.detach().contiguous(), key.detach().contiguous(), query_pos.detach().contiguous()
        ffn = self.decoder.linear1.out_features
        total_out = sum(self.head_out)
        ws_bytes = L.fnp_tf_decoder_workspace_bytes(B, K, N, ffn, total_out)
        if ws_bytes < 0:
            raise lib.FnpError(f"fnp_tf_decoder_workspace_bytes({B}, {K}, {N}, {ffn}, {total_out}) failed")
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev)
        out_feat = torch.empty((B, D_MODEL, K), dtype=torch.float32, device=dev)
        out_heads = torch.empty((B * K * total_out,), dtype=torch.float32, device=dev) if total_out else None
        batched = int(self.key_pe.shape[0] == B and B > 1)
        lib.check(L.fnp_tf_decoder(lib.ptr(query), lib.ptr(key), lib.ptr(query_pos), lib.ptr(self.key_pe), batched, lib.ptr(self.params),
                                   self.params.numel(), B, K, N, ffn, len(self.head_out), self.head_out_c, self.center, lib.ptr(ws),
                                   ws_bytes, lib.ptr(out_feat), lib.ptr(out_heads), lib.stream()), "fnp_tf_decoder")
        res, at = {}, 0
        for name, n_out in zip(self.names, self.head_out):
            res[name] = out_heads[at:at + B * n_out * K].view(B, n_out, K)
            at += B * n_out * K
        return out_feat, res


class DecoderHead:
    """decoder: a model_utils.transfusion_utils.TransformerDecoderLayer; prediction_head: a SeparateHead_Transfusion.

    __call__(query_feat (B, 128, K), lidar_feat_flatten (B, 128, H*W), query_pos (B, K, 2), bev_pos ([1 or B,] H*W, 2), all in
    xy as predict holds them behind its flips) -> the reference's res_layer dict, `center` already offset by query_pos.
    Pass the same bev_pos tensor on every call: the key position embedding is cached on it."""

    def __init__(self, decoder, prediction_head):
        self.decoder, self.prediction_head = decoder, prediction_head
        self.pack = DevicePack(decoder, prediction_head)

    def plain_reasons(self, query_feat, lidar_feat_flatten, query_pos, bev_pos):
        return self.pack.reasons(query_feat, lidar_feat_flatten, query_pos, bev_pos)

    def call_plain(self, query_feat, lidar_feat_flatten, query_pos, bev_pos):
        """transfusion_head.py:315-319 with the two modules called plainly (the decoder by forward_plain)"""
        B = query_feat.shape[0]
        pos = bev_pos if bev_pos.dim() == 3 else bev_pos[None]
        query_feat = self.decoder.forward_plain(query_feat, lidar_feat_flatten, query_pos, pos.expand(B, -1, -1))
        res_layer = self.prediction_head(query_feat)
        res_layer["center"] = res_layer["center"] + query_pos.permute(0, 2, 1)
        return res_layer

    def __call__(self, query_feat, lidar_feat_flatten, query_pos, bev_pos):
        if self.plain_reasons(query_feat, lidar_feat_flatten, query_pos, bev_pos):
            return self.call_plain(query_feat, lidar_feat_flatten, query_pos, bev_pos)
        return self.pack.run(query_feat, lidar_feat_flatten, query_pos, bev_pos)[1]
