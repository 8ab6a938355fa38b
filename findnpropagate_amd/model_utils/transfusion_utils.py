"""pcdet/models/model_utils/transfusion_utils.py:5-7 with the reference's signature (plain torch)."""
import torch


def clip_sigmoid(x, eps=1e-4):
    """clamp(sigmoid(x), eps, 1 - eps).  As in the reference the sigmoid is taken IN PLACE: x holds sigmoid(x) afterwards.
    utils.loss_utils.heatmap_loss, the fused path, leaves its logits alone."""
    y = torch.clamp(x.sigmoid_(), min=eps, max=1 - eps)
    return y
