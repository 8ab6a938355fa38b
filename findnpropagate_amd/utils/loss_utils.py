"""The heatmap loss of TransFusionHead (pcdet/utils/loss_utils.py:729-760 and transfusion_head.py:492-498).

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
