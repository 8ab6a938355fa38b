"""Dense heatmap targets of TransFusionHead on the device (pcdet/models/dense_heads/transfusion_head.py:446-470, batched over
get_targets' scenes :352-375).  The reference draws one ground-truth box at a time from Python — gaussian_radius on one-element
tensors, a numpy Gaussian, an upload and a clipped torch.max per box, with several device-to-host reads; here the batch is two
kernels (fnp_heatmap_box_params, fnp_heatmap_draw; csrc/heatmap.hip) and no host read.  Of the head this is the only slice in
the code base: the assignment, the decoder and the query initialisation stay with the reference."""
import numpy as np
import torch

from .. import lib


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


class HeatmapTargets:
    """target_assigner_cfg: the head's TARGET_ASSIGNER_CONFIG (a dict or an attribute dict): FEATURE_MAP_STRIDE,
    GAUSSIAN_OVERLAP, MIN_RADIUS, UNK_RADIUS_MULT (1 when absent).  grid_size (3) voxels x, y, z; point_cloud_range (6);
    voxel_size (3); unknown_labels: the 1-based labels of pseudo_processor.unknown_labels when the head runs with use_pseudo,
    () otherwise.

    __call__(gt_boxes (B, M, ncol) f32 device, label in the last column, 1-based, 0 = padding) ->
    (heatmap (B, C, H, W) f32 with H = grid_size[1] // stride along y and W = grid_size[0] // stride along x, num_pos (1,) int32:
    the count of targets equal to 1, on the device), and with return_params=True also params (B, M, 4) int32
    {class, cx, cy, r}, class -1 for a skipped row (a side <= 0, a non-finite x, y or side, a label outside 1..C: the reference
    raises on a label above C and wraps on one below 1, which is out of contract here).

    Parity is with the reference run on the CPU, bit for bit; the Gaussian weights are proven equal for radii up to 128."""

    def __init__(self, target_assigner_cfg, grid_size, point_cloud_range, voxel_size, num_classes, unknown_labels=()):
        self.stride = int(_get(target_assigner_cfg, "FEATURE_MAP_STRIDE"))
        self.overlap = float(_get(target_assigner_cfg, "GAUSSIAN_OVERLAP"))
        self.min_radius = int(_get(target_assigner_cfg, "MIN_RADIUS"))
        self.unk_mult = float(_get(target_assigner_cfg, "UNK_RADIUS_MULT", 1))
        self.num_classes = int(num_classes)
        assert 1 <= self.num_classes <= 64, "the unknown labels cross the ABI as a 64-bit mask"
        grid = [int(g) for g in np.asarray(grid_size).reshape(-1)[:2]]
        self.W, self.H = grid[0] // self.stride, grid[1] // self.stride
        self.voxel = [float(v) for v in np.asarray(voxel_size, dtype=np.float64).reshape(-1)[:2]]
        self.origin = [float(v) for v in np.asarray(point_cloud_range, dtype=np.float64).reshape(-1)[:2]]
        self.unk_mask = 0
        for label in unknown_labels:
            if 1 <= int(label) <= self.num_classes:
                self.unk_mask |= 1 << (int(label) - 1)

    def __call__(self, gt_boxes, return_params=False, out=None):
        L = lib.load()
        lib.require_device(gt_boxes)
        assert gt_boxes.dim() == 3 and gt_boxes.dtype == torch.float32 and (gt_boxes.shape[1] == 0 or gt_boxes.shape[2] >= 6), \
            "gt_boxes: (B, M, ncol) float32, label last"
        gt_boxes = gt_boxes.contiguous()
        B, M, ncol = (int(s) for s in gt_boxes.shape)
        dev, C, H, W = gt_boxes.device, self.num_classes, self.H, self.W
        s = lib.stream()
        params = torch.empty((B, M, 4), dtype=torch.int32, device=dev)
        heatmap = out if out is not None else torch.empty((B, C, H, W), dtype=torch.float32, device=dev)
        assert heatmap.shape == (B, C, H, W) and heatmap.dtype == torch.float32 and heatmap.is_contiguous()
        num_pos = torch.empty(1, dtype=torch.int32, device=dev)
        if B * M:
            lib.check(L.fnp_heatmap_box_params(lib.ptr(gt_boxes), B, M, ncol, C, self.voxel[0], self.voxel[1], self.stride,
                                               self.origin[0], self.origin[1], self.overlap, self.min_radius, self.unk_mask,
                                               self.unk_mult, lib.ptr(params), s), "fnp_heatmap_box_params")
        ws_bytes = L.fnp_heatmap_draw_workspace_bytes(B, C, H, W)
        if ws_bytes < 0:
            raise lib.FnpError(f"fnp_heatmap_draw_workspace_bytes({B}, {C}, {H}, {W}) failed")
        ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
        lib.check(L.fnp_heatmap_draw(lib.ptr(params), B, M, C, H, W, lib.ptr(ws), ws_bytes, lib.ptr(heatmap), lib.ptr(num_pos), s),
                  "fnp_heatmap_draw")
        return (heatmap, num_pos, params) if return_params else (heatmap, num_pos)
