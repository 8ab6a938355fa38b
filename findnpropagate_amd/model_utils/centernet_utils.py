"""Plain torch / numpy mirrors of pcdet/models/model_utils/centernet_utils.py:9-69 with the reference's signatures: drop-in use
on any device, the CPU yardstick of tests/test_heatmap_ref.py and the baseline of tools/bench_heatmap.py.  The hot path is
dense_heads.transfusion_targets.HeatmapTargets (fnp_heatmap_box_params + fnp_heatmap_draw), which replaces the per-box loop
built on these."""
import numpy as np
import torch


def gaussian_radius(height, width, min_overlap=0.5):
    """height, width: (N) tensors -> (N) the smallest of the three roots (CornerNet's radius)"""
    a1 = 1
    b1 = (height + width)
    c1 = width * height * (1 - min_overlap) / (1 + min_overlap)
    sq1 = (b1 ** 2 - 4 * a1 * c1).sqrt()
    r1 = (b1 + sq1) / 2

    a2 = 4
    b2 = 2 * (height + width)
    c2 = (1 - min_overlap) * width * height
    sq2 = (b2 ** 2 - 4 * a2 * c2).sqrt()
    r2 = (b2 + sq2) / 2

    a3 = 4 * min_overlap
    b3 = -2 * min_overlap * (height + width)
    c3 = (min_overlap - 1) * width * height
    sq3 = (b3 ** 2 - 4 * a3 * c3).sqrt()
    r3 = (b3 + sq3) / 2
    return torch.min(torch.min(r1, r2), r3)


def gaussian2D(shape, sigma=1):
    m, n = [(ss - 1.) / 2. for ss in shape]
    y, x = np.ogrid[-m:m + 1, -n:n + 1]
    h = np.exp(-(x * x + y * y) / (2 * sigma * sigma))
    h[h < np.finfo(h.dtype).eps * h.max()] = 0
    return h


def draw_gaussian_to_heatmap(heatmap, center, radius, k=1, valid_mask=None):
    """elementwise maximum of heatmap (H, W) with the (2 radius + 1)^2 Gaussian around center (x, y), clipped to the map"""
    diameter = 2 * radius + 1
    gaussian = gaussian2D((diameter, diameter), sigma=diameter / 6)
    x, y = int(center[0]), int(center[1])
    height, width = heatmap.shape[0:2]
    left, right = min(x, radius), min(width - x, radius + 1)
    top, bottom = min(y, radius), min(height - y, radius + 1)
    masked_heatmap = heatmap[y - top:y + bottom, x - left:x + right]
    masked_gaussian = torch.from_numpy(gaussian[radius - top:radius + bottom, radius - left:radius + right]).to(heatmap.device).float()
    if min(masked_gaussian.shape) > 0 and min(masked_heatmap.shape) > 0:
        if valid_mask is not None:
            cur_valid_mask = valid_mask[y - top:y + bottom, x - left:x + right]
            masked_gaussian = masked_gaussian * cur_valid_mask.float()
        torch.max(masked_heatmap, masked_gaussian * k, out=masked_heatmap)
    return heatmap
