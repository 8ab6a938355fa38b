"""The losses of TransFusionHead: the heatmap loss (pcdet/utils/loss_utils.py:729-760 and transfusion_head.py:492-498) and, at the
end of the file, the two losses behind the per-query targets (query_loss, query_loss_plain).

  GaussianFocalLoss   the reference's module, plain torch, per-element loss
  heatmap_loss        loss_heatmap(clip_sigmoid(dense_heatmap), heatmap).sum() / max(num_pos, 1): on device tensors with the
                      default alpha and gamma ONE forward pass and one backward kernel (fnp_heatmap_loss_forward / _backward,
                      csrc/heatmap.hip); otherwise the composition of the plain modules
"""
import torch
from torch import nn

from .. import lib
from ..model_utils.transfusion_utils import clip_sigmoid


class GaussianFocalLoss(nn.Module):
    """Focal loss against a Gaussian heatmap target (CornerNet): alpha the power of the prediction, gamma the power of
    (1 - target) on the negatives.  forward(pred, target) returns the per-element loss."""

    def __init__(self, alpha=2.0, gamma=4.0):
        super().__init__()
        self.alpha = alpha
        self.gamma = gamma

    def forward(self, pred, target):
        eps = 1e-12
        pos_weights = target.eq(1)
        neg_weights = (1 - target).pow(self.gamma)
        pos_loss = -(pred + eps).log() * (1 - pred).pow(self.alpha) * pos_weights
        neg_loss = -(1 - pred + eps).log() * pred.pow(self.alpha) * neg_weights
        return pos_loss + neg_loss


class _HeatmapLoss(torch.autograd.Function):
    """forward: two launches (partial sums, finish); backward: one elementwise kernel that recomputes the derivative from the
    saved logits and targets.  Nothing synchronises: num_pos and the incoming gradient are read from device memory."""

    @staticmethod
    def forward(ctx, logits, target, num_pos):
        L = lib.load()
        x = logits.detach().contiguous()
        t = target.detach().to(torch.float32).contiguous()
        n = x.numel()
        ws_bytes = L.fnp_heatmap_loss_workspace_bytes(n)
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        lib.check(L.fnp_heatmap_loss_forward(lib.ptr(x), lib.dtype_code(x), lib.ptr(t), n, lib.ptr(num_pos), lib.ptr(ws), ws_bytes,
                                             lib.ptr(loss), lib.stream()), "fnp_heatmap_loss_forward")
        ctx.save_for_backward(x, t, num_pos)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        x, t, num_pos = ctx.saved_tensors
        g = grad_out.detach().to(torch.float32).contiguous()
        grad = torch.empty_like(x)
        lib.check(lib.load().fnp_heatmap_loss_backward(lib.ptr(x), lib.dtype_code(x), lib.ptr(t), x.numel(), lib.ptr(num_pos), lib.ptr(g),
                                                       lib.ptr(grad), lib.stream()), "fnp_heatmap_loss_backward")
        return grad, None, None


def heatmap_loss(dense_heatmap, heatmap, num_pos=None, loss_fn=None):
    """loss_heatmap(clip_sigmoid(dense_heatmap), heatmap).sum() / max(num_pos, 1) as a 0-dim f32 tensor (transfusion_head.py:493-496).

    dense_heatmap: logits (B, C, H, W), f32, f16 or bf16; heatmap: targets of the same shape (HeatmapTargets); num_pos: the
    count of targets equal to 1 as a one-element int32 device tensor (HeatmapTargets returns it), or None: counted here, on the
    device.  The result stays on the device — the reference's .item() calls are the caller's to make, if it wants them.
    NOT MIRRORED: the reference's clip_sigmoid overwrites dense_heatmap with its sigmoid (nothing reads it afterwards); here
    the logits are left as they are.
    loss_fn: a GaussianFocalLoss; anything but the default alpha = 2, gamma = 4, or a CPU tensor, takes the plain composition."""
    default = loss_fn is None or (isinstance(loss_fn, GaussianFocalLoss) and loss_fn.alpha == 2.0 and loss_fn.gamma == 4.0)
    if dense_heatmap.is_cuda and default:
        assert heatmap.shape == dense_heatmap.shape, "logits and targets differ in shape"
        lib.require_device(heatmap, num_pos)
        if num_pos is None:
            num_pos = heatmap.eq(1).sum().to(torch.int32)
        assert num_pos.dtype == torch.int32 and num_pos.numel() == 1, "num_pos: one int32"
        return _HeatmapLoss.apply(dense_heatmap, heatmap, num_pos.reshape(1))
    loss_fn = loss_fn or GaussianFocalLoss()
    n = heatmap.eq(1).float().sum() if num_pos is None else num_pos.reshape(()).float()
    return loss_fn(clip_sigmoid(dense_heatmap.clone()), heatmap).sum() / n.clamp(min=1)


# ---- the two losses behind the per-query targets (transfusion_head.py:500-504, :561-597) ------------------------------------------
#   query_loss        (loss_cls, loss_bbox), unweighted as heatmap_loss is (the caller applies cls_weight and bbox_weight): on
#                     device tensors in the default configuration one forward pass with a finishing workgroup and one backward
#                     kernel (fnp_tf_query_loss_forward / _backward, csrc/tfassign.hip), the heads read where they lie
#   query_loss_plain  the same two numbers in plain torch from the formulas of include/fnp.h, differentiable by autograd: CPU
#                     tensors, other dtypes and every configuration outside the default

def _cfg_get(cfg, key, default=None):
    if cfg is None:
        return default
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def _query_loss_cfg(loss_cfg):
    """-> alpha, gamma, code_weights, unknown_code_weights or None, unknown_cls_weight or None, default (bool: the focal
    sigmoid loss without label smoothing or balanced reweighting, which is what the kernels cover)"""
    cls, w = _cfg_get(loss_cfg, "LOSS_CLS", {}), _cfg_get(loss_cfg, "LOSS_WEIGHTS", {})
    other = any(_cfg_get(cls, k, False) for k in ("use_poly1", "use_mae", "use_ce"))
    default = not other and not _cfg_get(loss_cfg, "LABEL_SMOOTHING", False) and not _cfg_get(loss_cfg, "BALANCED_REWEIGHTING", False)
    ucw = _cfg_get(w, "unknown_code_weights")
    return (float(_cfg_get(cls, "alpha", 0.25)), float(_cfg_get(cls, "gamma", 2.0)), [float(v) for v in _cfg_get(w, "code_weights")],
            None if ucw is None else [float(v) for v in ucw], _cfg_get(w, "unknown_cls_weight"), default)


def query_loss_plain(preds, targets, loss_cfg, head_order):
    """preds: the head outputs (B, n, K); targets: the dict of QueryTargets; -> (loss_cls, loss_bbox), 0-dim tensors."""
    alpha, gamma, code_w, unk_code_w, unk_cls_w, default = _query_loss_cfg(loss_cfg)
    if not default:
        raise NotImplementedError("query_loss covers SigmoidFocalClassificationLoss without label smoothing or balanced reweighting")
    x = preds["heatmap"].permute(0, 2, 1)                                        # (B, K, C)
    dt = x.dtype
    C = x.shape[-1]
    unk = targets["unknown_mask"].bool()
    t = (targets["labels"].unsqueeze(-1) == torch.arange(C, device=x.device)).to(dt)
    w = targets["label_weights"].float()                                         # (the weights are f32 tensors whatever the heads are)
    if unk_cls_w is not None:
        w = torch.where(unk, w * float(unk_cls_w), w)
    w = w.to(dt)
    p = torch.sigmoid(x)
    focal = (t * alpha + (1 - t) * (1 - alpha)) * (t * (1 - p) + (1 - t) * p).pow(gamma)
    bce = x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    den = targets["num_pos"].to(dt).clamp(min=1).reshape(())
    loss_cls = (focal * bce * w.unsqueeze(-1)).sum() / den
    pred = torch.cat([preds[h] for h in head_order], dim=1).permute(0, 2, 1)     # (B, K, code)
    rw = targets["bbox_weights"].float() * torch.tensor(code_w, dtype=torch.float32, device=x.device)
    if unk_code_w is not None:
        rw = torch.where(unk.unsqueeze(-1), rw * torch.tensor(unk_code_w, dtype=torch.float32, device=x.device), rw)
    rw = rw.to(dt)
    loss_bbox = ((pred - targets["bbox_targets"].to(dt)).abs() * rw).sum() / den
    return loss_cls, loss_bbox


class _QueryLoss(torch.autograd.Function):
    """forward: two launches (partial sums, finish); backward: one elementwise kernel.  Nothing synchronises: num_pos and the
    incoming gradients are read from device memory."""

    @staticmethod
    def forward(ctx, cfg, targets, heatmap, *heads):
        import ctypes
        L = lib.load()
        alpha, gamma, code_w, unk_code_w, unk_cls_w = cfg
        x = heatmap.detach().contiguous()
        hs = [h.detach().contiguous() for h in heads]
        B, C, K = (int(s) for s in x.shape)
        code = sum(int(h.shape[1]) for h in hs)
        assert len(code_w) == code and (unk_code_w is None or len(unk_code_w) == code), "code_weights: one per code channel"
        assert all(h.shape[0] == B and h.shape[2] == K for h in hs) and 1 <= len(hs) <= 8
        tens = [targets["labels"].contiguous(), targets["label_weights"].float().contiguous(), targets["bbox_targets"].float().contiguous(),
                targets["bbox_weights"].float().contiguous(), targets["unknown_mask"].contiguous().view(torch.uint8), targets["num_pos"]]
        assert tens[0].dtype == torch.int64 and tens[5].dtype == torch.int32 and tens[2].shape == (B, K, code)
        lib.require_device(x, *hs, *tens)
        abi = dict(ptrs=(ctypes.c_void_p * len(hs))(*(lib.ptr(h) for h in hs)), ch=(ctypes.c_int * len(hs))(*(int(h.shape[1]) for h in hs)),
                   cw=(ctypes.c_float * code)(*code_w), ucw=None if unk_code_w is None else (ctypes.c_float * code)(*unk_code_w),
                   shape=(len(hs), lib.dtype_code(x), B, C, K, code), scal=(alpha, gamma), ucls=1.0 if unk_cls_w is None else float(unk_cls_w))
        ws_bytes = L.fnp_tf_query_loss_workspace_bytes()
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=x.device)
        loss = torch.empty(2, dtype=torch.float32, device=x.device)
        lib.check(L.fnp_tf_query_loss_forward(lib.ptr(x), abi["ptrs"], abi["ch"], *abi["shape"], *(lib.ptr(t) for t in tens), *abi["scal"],
                                              abi["cw"], abi["ucw"], abi["ucls"], lib.ptr(ws), ws_bytes, lib.ptr(loss), lib.stream()),
                  "fnp_tf_query_loss_forward")
        ctx.save_for_backward(x, *hs, *tens)
        ctx.abi, ctx.n_heads = abi, len(hs)
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, g_cls, g_bbox):
        import ctypes
        saved = ctx.saved_tensors
        x, hs, tens, abi = saved[0], saved[1:1 + ctx.n_heads], saved[1 + ctx.n_heads:], ctx.abi
        g = torch.stack([g_cls.detach().float().reshape(()), g_bbox.detach().float().reshape(())]).contiguous()
        gx, ghs = torch.empty_like(x), [torch.empty_like(h) for h in hs]
        gptrs = (ctypes.c_void_p * len(hs))(*(lib.ptr(t) for t in ghs))
        lib.check(lib.load().fnp_tf_query_loss_backward(lib.ptr(x), abi["ptrs"], abi["ch"], *abi["shape"], *(lib.ptr(t) for t in tens),
                                                        *abi["scal"], abi["cw"], abi["ucw"], abi["ucls"], lib.ptr(g), lib.ptr(gx), gptrs,
                                                        lib.stream()), "fnp_tf_query_loss_backward")
        return (None, None, gx, *ghs)


def query_loss(preds, targets, loss_cfg, head_order):
    """(loss_cls, loss_bbox) of TransFusionHead.loss, each the sum over the batch divided by max(num_pos, 1), unweighted.
    preds: the head outputs (B, n, K), the logits under "heatmap"; targets: the dict QueryTargets returns; loss_cfg: the head's
    LOSS_CONFIG (LOSS_CLS {gamma, alpha}, LOSS_WEIGHTS {code_weights, unknown_code_weights, unknown_cls_weight}); head_order:
    SEPARATE_HEAD_CFG.HEAD_ORDER.  Device tensors of one dtype (f32, f16, bf16) in the default configuration run the kernels and
    read nothing back; CPU tensors take query_loss_plain; a configuration outside the default raises there."""
    alpha, gamma, code_w, unk_code_w, unk_cls_w, default = _query_loss_cfg(loss_cfg)
    heads = [preds[h] for h in head_order]
    x = preds["heatmap"]
    device = default and x.is_cuda and x.dtype in (torch.float32, torch.float16, torch.bfloat16) and \
        all(h.is_cuda and h.dtype == x.dtype for h in heads) and all(torch.is_tensor(v) and v.is_cuda for v in targets.values())
    if not device:
        return query_loss_plain(preds, targets, loss_cfg, head_order)
    return _QueryLoss.apply((alpha, gamma, code_w, unk_code_w, unk_cls_w), targets, x, *heads)
