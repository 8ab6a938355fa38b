"""Hungarian assignment and per-query targets of TransFusionHead on the device (pcdet/models/dense_heads/
transfusion_head.py:352-444 without the dense heatmap, target_assigner/hungarian_assigner.py:61-132).  Per scene the reference
tests every ground-truth row from Python, builds the cost in some thirty launches, copies it to the host for scipy's
linear_sum_assignment, copies the match back and loops over the positives; QueryTargets does the batch in four launches
(csrc/tfassign.hip) and reads nothing back.  hungarian_match is the matching alone, lsap_host its serial host twin; both
return scipy's own assignment, ties included (csrc/lsap.h states what fixes it).  CPU tensors take query_targets_plain.  The
two losses that consume the targets are utils.loss_utils.query_loss."""
import ctypes

import numpy as np
import torch

from .. import lib

MAX_QUERIES, MAX_BOXES = 2048, 1024


def hungarian_match(cost, num_valid, valid_map=None, iou=None):
    """cost (B, K, Mcap) f32 device, finite; scene b uses its K x num_valid[b] leading columns (num_valid (B) int32 device).
    -> assigned (B, K) int32: the matched box per query, -1 elsewhere, named by valid_map[b, column] ((B, Mcap) int32) or by
    the column itself; with iou (B, K, Mcap) f32 also matched_ious (B, K) f32: the IoU at the match clamped to [0, 1], else 0.
    K <= 2048, Mcap <= 1024.  No host read."""
    L = lib.load()
    lib.require_device(cost, num_valid, valid_map, iou)
    assert cost.dim() == 3 and cost.dtype == torch.float32, "cost: (B, K, Mcap) float32"
    B, K, M = (int(s) for s in cost.shape)
    assert K <= MAX_QUERIES and M <= MAX_BOXES, "fnp_tf_assign_match: K <= 2048, Mcap <= 1024"
    assert num_valid.shape == (B,) and num_valid.dtype == torch.int32
    assert valid_map is None or (valid_map.shape == (B, M) and valid_map.dtype == torch.int32)
    assert iou is None or (iou.shape == (B, K, M) and iou.dtype == torch.float32)
    cost, num_valid = cost.contiguous(), num_valid.contiguous()
    valid_map = None if valid_map is None else valid_map.contiguous()
    iou = None if iou is None else iou.contiguous()
    assigned = torch.empty((B, K), dtype=torch.int32, device=cost.device)
    matched = None if iou is None else torch.empty((B, K), dtype=torch.float32, device=cost.device)
    lib.check(L.fnp_tf_assign_match(lib.ptr(cost), lib.ptr(iou), lib.ptr(num_valid), lib.ptr(valid_map), B, K, M,
                                    lib.ptr(assigned), lib.ptr(matched), lib.stream()), "fnp_tf_assign_match")
    return assigned if iou is None else (assigned, matched)


def lsap_host(cost):
    """scipy.optimize.linear_sum_assignment(cost) for a 2-D f32 matrix on the host, by the library's serial solver
    (fnp_host_lsap) -> (rows, cols) int64 arrays, rows ascending."""
    L = lib.load()
    cost = np.ascontiguousarray(cost, dtype=np.float32)
    assert cost.ndim == 2
    nr, nc = cost.shape
    n = min(nr, nc)
    rows, cols = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    lib.check(L.fnp_host_lsap(cost.ctypes.data, nr, nc, rows.ctypes.data, cols.ctypes.data), "fnp_host_lsap")
    return rows.astype(np.int64), cols.astype(np.int64)


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


HEADS = ("heatmap", "center", "height", "dim", "rot", "vel")


class QueryTargets:
    """get_targets of TransFusionHead without its dense heatmap (transfusion_head.py:352-444; the heatmap is HeatmapTargets').

    target_assigner_cfg: the head's TARGET_ASSIGNER_CONFIG (a dict or an attribute dict): FEATURE_MAP_STRIDE and
    HUNGARIAN_ASSIGNER {cls_cost {weight, alpha, gamma, eps}, reg_cost {weight}, iou_cost {weight}} with the reference's
    defaults (0.15, 0.25, 2.0, 1e-12; 0.25; 0.25).  point_cloud_range (6), voxel_size (3); code_size 10 (with `vel`) or 8;
    unknown_labels: the 1-based labels of pseudo_processor.unknown_labels when the head runs with use_pseudo, () otherwise.

    __call__(preds, gt_boxes (B, Mcap, code_size) f32 device, label last, 1-based, 0 = padding): preds holds the head outputs
    heatmap (logits, B, C, K), center, height, dim, rot and, for code_size 10, vel, f32, detached here as the reference does ->
    dict of labels (B, K) int64, label_weights (B, K) f32, bbox_targets and bbox_weights (B, K, code_size) f32, unknown_mask
    (B, K) bool, num_pos (1,) int32 ON THE DEVICE, assigned (B, K) int32 (row of gt_boxes or -1), matched_ious (B, K) f32 and,
    with return_debug, cost, iou (B, K, Mcap), boxes (B, K, code_size - 1), num_valid (B), valid_map (B, Mcap).
    Four launches (fnp_tf_assign_cost: 2, fnp_tf_assign_match, fnp_tf_assign_targets) and no host read.  CPU tensors take the
    plain route, query_targets_plain."""

    def __init__(self, target_assigner_cfg, point_cloud_range, voxel_size, num_classes, code_size=10, unknown_labels=()):
        self.stride = int(_get(target_assigner_cfg, "FEATURE_MAP_STRIDE"))
        ha = _get(target_assigner_cfg, "HUNGARIAN_ASSIGNER", {}) or {}
        cls, reg, iou = (_get(ha, k, {}) or {} for k in ("cls_cost", "reg_cost", "iou_cost"))
        self.cls_weight = float(_get(cls, "weight", 0.15))
        self.alpha, self.gamma, self.eps = float(_get(cls, "alpha", 0.25)), float(_get(cls, "gamma", 2.0)), float(_get(cls, "eps", 1e-12))
        self.reg_weight, self.iou_weight = float(_get(reg, "weight", 0.25)), float(_get(iou, "weight", 0.25))
        self.num_classes, self.code_size = int(num_classes), int(code_size)
        assert 1 <= self.num_classes <= 64 and self.code_size in (8, 10)
        self.range = [float(np.float32(v)) for v in np.asarray(point_cloud_range, dtype=np.float64).reshape(-1)[:6]]
        self.voxel = [float(v) for v in np.asarray(voxel_size, dtype=np.float64).reshape(-1)[:2]]
        self.unknown_labels = tuple(int(v) for v in unknown_labels)
        self.unk_mask = 0
        for label in self.unknown_labels:
            if 1 <= label <= self.num_classes:
                self.unk_mask |= 1 << (label - 1)

    def __call__(self, preds, gt_boxes, return_debug=False):
        if not gt_boxes.is_cuda or not all(preds[k].is_cuda for k in HEADS if k in preds):
            return query_targets_plain(self, preds, gt_boxes, return_debug)      # CPU tensors: the plain route
        L = lib.load()
        heads = [preds[k].detach().contiguous() if k in preds else None for k in HEADS]
        hm = heads[0]
        B, C, K = (int(s) for s in hm.shape)
        code = self.code_size
        assert C == self.num_classes and all(h is None or h.dtype == torch.float32 for h in heads)
        assert gt_boxes.dim() == 3 and gt_boxes.shape[0] == B and gt_boxes.shape[2] == code and gt_boxes.dtype == torch.float32
        assert (code == 10) == (heads[5] is not None), "code_size 10 goes with a `vel` head, 8 with none"
        gt_boxes = gt_boxes.contiguous()
        M, dev, s = int(gt_boxes.shape[1]), hm.device, lib.stream()
        assert K <= MAX_QUERIES and M <= MAX_BOXES
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        num_valid, valid_map = torch.empty(B, **i32), torch.empty((B, M), **i32)
        cost, iou, boxes = torch.empty((B, K, M), **f32), torch.empty((B, K, M), **f32), torch.empty((B, K, code - 1), **f32)
        rng = (ctypes.c_float * 6)(*self.range)
        lib.check(L.fnp_tf_assign_cost(*(lib.ptr(h) for h in heads), lib.ptr(gt_boxes), B, C, K, M, code, self.stride,
                                       self.voxel[0], self.voxel[1], rng, self.cls_weight, self.alpha, self.gamma, self.eps,
                                       self.reg_weight, self.iou_weight, lib.ptr(num_valid), lib.ptr(valid_map), lib.ptr(cost),
                                       lib.ptr(iou), lib.ptr(boxes), s), "fnp_tf_assign_cost")
        assigned, matched = torch.empty((B, K), **i32), torch.empty((B, K), **f32)
        lib.check(L.fnp_tf_assign_match(lib.ptr(cost), lib.ptr(iou), lib.ptr(num_valid), lib.ptr(valid_map), B, K, M,
                                        lib.ptr(assigned), lib.ptr(matched), s), "fnp_tf_assign_match")
        labels = torch.empty((B, K), dtype=torch.int64, device=dev)
        label_weights = torch.empty((B, K), **f32)
        bbox_targets, bbox_weights = torch.empty((B, K, code), **f32), torch.empty((B, K, code), **f32)
        unknown = torch.empty((B, K), dtype=torch.uint8, device=dev)
        num_pos = torch.empty(1, **i32)
        lib.check(L.fnp_tf_assign_targets(lib.ptr(assigned), lib.ptr(gt_boxes), B, C, K, M, code, self.stride, self.voxel[0],
                                          self.voxel[1], self.range[0], self.range[1], self.unk_mask, lib.ptr(labels),
                                          lib.ptr(label_weights), lib.ptr(bbox_targets), lib.ptr(bbox_weights), lib.ptr(unknown),
                                          lib.ptr(num_pos), s), "fnp_tf_assign_targets")
        out = dict(labels=labels, label_weights=label_weights, bbox_targets=bbox_targets, bbox_weights=bbox_weights,
                   unknown_mask=unknown.view(torch.bool), num_pos=num_pos, assigned=assigned, matched_ious=matched)
        if return_debug:
            out.update(cost=cost, iou=iou, boxes=boxes, num_valid=num_valid, valid_map=valid_map)
        return out



def _bev_overlap(q, g):
    """(K, 7+), (M, 7+) -> (K, M) BEV overlap areas by the library: its kernel on device tensors, its host twin on CPU tensors"""
    a, b = q[:, :7].float().contiguous(), g[:, :7].float().contiguous()
    out = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    L = lib.load()
    if a.is_cuda:
        lib.check(L.fnp_boxes_overlap_bev(lib.ptr(a), a.shape[0], lib.ptr(b), b.shape[0], lib.ptr(out), lib.stream()), "fnp_boxes_overlap_bev")
    else:
        lib.check(L.fnp_host_boxes_overlap_bev(lib.ptr(a), a.shape[0], lib.ptr(b), b.shape[0], lib.ptr(out)), "fnp_host_boxes_overlap_bev")
    return out.to(q.dtype)


def query_targets_plain(qt, preds, gt_boxes, return_debug=False):
    """What QueryTargets computes, in plain torch, scene by scene, written from the formulas of include/fnp.h: for CPU tensors
    (QueryTargets.__call__ routes them here), for any float dtype (f64 heads give an f64 evaluation), and as the comparison
    span of tools/bench_assign.py.  It reads back per scene: the valid rows, and the cost for the host solver (fnp_host_lsap).
    Same keys as QueryTargets; with return_debug, cost / iou / boxes are per-scene lists over the valid columns."""
    hm = preds["heatmap"].detach()
    B, C, K = (int(s) for s in hm.shape)
    code, dt, dev = qt.code_size, hm.dtype, hm.device
    lo = torch.tensor(qt.range[0:2], dtype=dt, device=dev)
    extent = torch.tensor(qt.range[3:5], dtype=dt, device=dev) - lo
    cell_f64 = [qt.stride * qt.voxel[0], qt.stride * qt.voxel[1]]
    cell = torch.tensor(cell_f64, dtype=dt, device=dev)
    voxel = torch.tensor(qt.voxel[0:2], dtype=dt, device=dev)
    out = dict(labels=torch.full((B, K), C, dtype=torch.int64, device=dev), label_weights=torch.ones((B, K), dtype=torch.float32, device=dev),
               bbox_targets=torch.zeros((B, K, code), dtype=dt, device=dev), bbox_weights=torch.zeros((B, K, code), dtype=dt, device=dev),
               unknown_mask=torch.zeros((B, K), dtype=torch.bool, device=dev), assigned=torch.full((B, K), -1, dtype=torch.int32, device=dev),
               matched_ious=torch.zeros((B, K), dtype=dt, device=dev))
    dbg = dict(cost=[], iou=[], boxes=[], num_valid=[], valid_map=[])
    unknown = torch.tensor(sorted(qt.unknown_labels), dtype=torch.int64, device=dev)
    total = 0
    for b in range(B):
        g = gt_boxes[b].to(dt)
        lab = g[:, -1]
        ok = (g[:, 3] > 0) & (g[:, 4] > 0) & (lab >= 1) & (lab < C + 1) & torch.isfinite(g[:, 0]) & torch.isfinite(g[:, 1]) \
            & torch.isfinite(g[:, 3]) & torch.isfinite(g[:, 4])
        rows = torch.nonzero(ok).flatten()                                           # (a host read)
        h = {k: v[b].detach() for k, v in preds.items()}
        xy = h["center"] * qt.stride * voxel[:, None] + lo[:, None]
        parts = [xy, h["height"], h["dim"].exp(), torch.atan2(h["rot"][0:1], h["rot"][1:2])] + ([h["vel"]] if code == 10 else [])
        q = torch.cat(parts, 0).T.contiguous()                                       # (K, 7 or 9)
        g = g[rows]
        M = int(rows.numel())
        p = hm[b].sigmoid().T[:, g[:, -1].long() - 1]                                # (K, M)
        one_m = 1 - p
        pos = -(p + qt.eps).log() * qt.alpha * one_m.pow(qt.gamma)
        neg = -(one_m + qt.eps).log() * (1 - qt.alpha) * p.pow(qt.gamma)
        nq, ng = (q[:, 0:2] - lo) / extent, (g[:, 0:2] - lo) / extent
        reg = (nq[:, None, :] - ng[None, :, :]).abs().sum(-1)
        z_hi = torch.min((q[:, 2] + q[:, 5])[:, None], (g[:, 2] + g[:, 5])[None])
        z_lo = torch.max(q[:, 2][:, None], g[:, 2][None])
        o3 = (_bev_overlap(q, g) if M else q.new_zeros((K, 0))) * (z_hi - z_lo).clamp(min=0)
        union = (q[:, 3] * q[:, 4] * q[:, 5])[:, None] + (g[:, 3] * g[:, 4] * g[:, 5])[None] - o3
        iou = o3 / union.clamp(min=1e-8)
        cost = (pos - neg) * qt.cls_weight + reg * qt.reg_weight + (-iou) * qt.iou_weight
        for k, v in (("cost", cost), ("iou", iou), ("boxes", q), ("num_valid", M), ("valid_map", rows)):
            dbg[k].append(v)
        if not M:
            continue
        qi, gi = lsap_host(cost.detach().float().cpu().numpy())                      # (a host read)
        qi, gi = torch.from_numpy(qi).to(dev), torch.from_numpy(gi).to(dev)
        m = g[gi]
        t = [(m[:, 0:2] - lo) / cell, m[:, 2:3], m[:, 3:6].log(), m[:, 6:7].sin(), m[:, 6:7].cos()] + ([m[:, 7:9]] if code == 10 else [])
        out["bbox_targets"][b, qi] = torch.cat(t, 1)
        out["bbox_weights"][b, qi] = 1
        out["labels"][b, qi] = m[:, -1].long() - 1
        out["unknown_mask"][b, qi] = torch.isin(m[:, -1].long(), unknown)
        out["assigned"][b, qi] = rows[gi].to(torch.int32)
        out["matched_ious"][b, qi] = iou[qi, gi].clamp(0, 1)
        total += int(qi.numel())
    out["num_pos"] = torch.tensor([total], dtype=torch.int32, device=dev)
    if return_debug:
        out.update(dbg)
    return out
