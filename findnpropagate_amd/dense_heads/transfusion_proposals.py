"""Inference side of TransFusionHead around its decoder, on the device (pcdet/models/dense_heads/transfusion_head.py): the
heatmap proposals of predict (:201-294, :321-324), the query initialisation (:295-313) and get_bboxes + decode_bbox(filter=True)
(:616-728).  The reference spends a full-map sigmoid, a max_pool2d, a full argsort of C*H*W values per scene, a one-hot Conv1d,
about twenty small launches in the decode and a Python loop with an .item() per query; here the proposals are three launches
(csrc/proposals.hip), the query initialisation one and the decode one, with no host read.  The nn.Module head, the decoder,
the prediction heads and the assignment stay with the reference.

proposals_plain / init_queries_plain / get_bboxes_plain are the same spans as plain torch ops: what tools/bench_proposals.py
times against, and what init_queries runs on the device-selected indices when autograd is recording."""
import ctypes

import torch
import torch.nn.functional as F

from .. import lib

MAX_PROPOSALS = 2048      # kMaxK of csrc/proposals.hip


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def point_classes(dataset_name, num_classes, class_names=None):
    """the classes whose every cell stays a candidate (transfusion_head.py:264-280)"""
    if dataset_name == "nuScenes" and num_classes == 10:
        return [8, 9]
    if dataset_name == "Waymo":
        return [1, 2]
    if dataset_name == "kitti":
        assert class_names is not None, "kitti: class_names select the point classes"
        return [i for i, name in enumerate(class_names) if name in ("Pedestrian", "Person_Sitting", "Cyclist")]
    return []


def check_heatmap(dense_heatmap, num_classes, num_proposals):
    """host-side argument checks of HeatmapProposals.__call__ (no library needed)"""
    assert isinstance(dense_heatmap, torch.Tensor) and dense_heatmap.dim() == 4, "dense_heatmap: (B, C, H, W)"
    assert dense_heatmap.dtype == torch.float32, f"dense_heatmap must be float32, got {dense_heatmap.dtype}"
    B, C, H, W = (int(s) for s in dense_heatmap.shape)
    assert C == num_classes, f"dense_heatmap has {C} classes, the head {num_classes}"
    assert H >= 1 and W >= 1 and C * H * W < 2 ** 31 - 1, "C*H*W must be in [1, 2^31)"
    assert num_proposals <= C * H * W, f"num_proposals {num_proposals} exceeds C*H*W = {C * H * W}"
    return B, C, H, W


class HeatmapProposals:
    """num_proposals (K, at most 2048), nms_kernel_size (must be 3: with 1 the reference's own [padding:-padding] slice is
    empty), num_classes (1..64: the point classes cross the ABI as a 64-bit mask), dataset_name and, for kitti, class_names.

    __call__(dense_heatmap (B, C, H, W) f32 on the device, from_logits=True) -> top_class, top_index (B, K) int64,
    top_score (B, K) f32, query_heatmap_score (B, C, K) f32.  from_logits=False takes probabilities >= 0, as
    dense_heatmap.detach().sigmoid().  Order: masked value descending, then flat index ascending (the reference's argsort is
    not stable; on distinct values the two agree); masked-out cells take part with value 0 and fill the places behind the
    positive ones with the lowest flat indices.  NaN is out of contract.  No gradient: the reference detaches here."""

    def __init__(self, num_proposals, nms_kernel_size, num_classes, dataset_name, class_names=None):
        assert int(nms_kernel_size) == 3, f"NMS_KERNEL_SIZE must be 3, got {nms_kernel_size}"
        self.num_proposals, self.num_classes = int(num_proposals), int(num_classes)
        assert 1 <= self.num_classes <= 64, "the point classes cross the ABI as a 64-bit mask: 1 <= num_classes <= 64"
        assert 1 <= self.num_proposals <= MAX_PROPOSALS, f"1 <= num_proposals <= {MAX_PROPOSALS}"
        self.dataset_name = dataset_name
        self.point_classes = point_classes(dataset_name, self.num_classes, class_names)
        self.point_mask = 0
        for c in self.point_classes:
            assert 0 <= c < self.num_classes
            self.point_mask |= 1 << c

    def __call__(self, dense_heatmap, from_logits=True, out=None):
        B, C, H, W = check_heatmap(dense_heatmap, self.num_classes, self.num_proposals)
        K = self.num_proposals
        L = lib.load()
        lib.require_device(dense_heatmap)
        heat = dense_heatmap.detach().contiguous()
        dev = heat.device
        if out is None:
            out = (torch.empty((B, K), dtype=torch.int64, device=dev), torch.empty((B, K), dtype=torch.int64, device=dev),
                   torch.empty((B, K), dtype=torch.float32, device=dev), torch.empty((B, C, K), dtype=torch.float32, device=dev))
        top_class, top_index, top_score, qhs = out
        assert top_class.shape == (B, K) and top_index.shape == (B, K) and top_score.shape == (B, K) and qhs.shape == (B, C, K)
        assert top_class.dtype == torch.int64 and top_index.dtype == torch.int64 and top_score.dtype == qhs.dtype == torch.float32
        if B == 0:
            return top_class, top_index, top_score, qhs
        ws_bytes = L.fnp_proposals_workspace_bytes(B, C, H, W, K)
        if ws_bytes < 0:
            raise lib.FnpError(f"fnp_proposals_workspace_bytes({B}, {C}, {H}, {W}, {K}) failed")
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
        lib.check(L.fnp_proposals(lib.ptr(heat), B, C, H, W, K, int(bool(from_logits)), self.point_mask, lib.ptr(ws), ws_bytes,
                                  lib.ptr(top_class), lib.ptr(top_index), lib.ptr(top_score), lib.ptr(qhs), lib.stream()),
                  "fnp_proposals")
        return top_class, top_index, top_score, qhs

    def init_queries(self, lidar_feat_flatten, bev_pos, enc_weight, enc_bias, top_class, top_index):
        """lidar_feat_flatten (B, F, H*W); bev_pos (H*W, 2), (1, H*W, 2) or (B, H*W, 2): the head's own table, whose row order
        is create_2D_grid's (positions are never recomputed from the index); enc_weight (F, C) or the Conv1d's (F, C, 1);
        enc_bias (F) -> query_feat (B, F, K) = the gathered features + (weight column of the class + bias), query_pos (B, K, 2)
        = the gathered rows flipped to xy.  When autograd is recording and an input requires grad, the same span runs as plain
        torch ops on the given indices, so training keeps its gradient."""
        check_init_queries(lidar_feat_flatten, bev_pos, enc_weight, enc_bias, top_class, top_index, self.num_classes)
        if torch.is_grad_enabled() and any(t.requires_grad for t in (lidar_feat_flatten, bev_pos, enc_weight, enc_bias)):
            return init_queries_plain(lidar_feat_flatten, bev_pos, enc_weight, enc_bias, top_class, top_index)
        L = lib.load()
        lib.require_device(lidar_feat_flatten, bev_pos, enc_weight, enc_bias, top_class, top_index)
        B, Fd, HW = (int(s) for s in lidar_feat_flatten.shape)
        K = int(top_index.shape[1])
        dev = lidar_feat_flatten.device
        feat, pos = lidar_feat_flatten.detach().contiguous(), bev_pos.detach().contiguous()
        w = enc_weight.detach().reshape(Fd, self.num_classes).contiguous()
        bias = enc_bias.detach().contiguous()
        batched = int(pos.dim() == 3 and pos.shape[0] == B and B > 1)
        query_feat = torch.empty((B, Fd, K), dtype=torch.float32, device=dev)
        query_pos = torch.empty((B, K, 2), dtype=torch.float32, device=dev)
        if B:
            lib.check(L.fnp_query_init(lib.ptr(feat), lib.ptr(pos), batched, lib.ptr(w), lib.ptr(bias), lib.ptr(top_class.contiguous()),
                                       lib.ptr(top_index.contiguous()), B, Fd, HW, self.num_classes, K, lib.ptr(query_feat),
                                       lib.ptr(query_pos), lib.stream()), "fnp_query_init")
        return query_feat, query_pos


def check_init_queries(lidar_feat_flatten, bev_pos, enc_weight, enc_bias, top_class, top_index, num_classes):
    assert lidar_feat_flatten.dim() == 3 and lidar_feat_flatten.dtype == torch.float32, "lidar_feat_flatten: (B, F, H*W) float32"
    B, Fd, HW = (int(s) for s in lidar_feat_flatten.shape)
    assert Fd >= 2, "at least two feature channels"
    assert bev_pos.dtype == torch.float32 and bev_pos.shape[-2:] == (HW, 2) and \
        (bev_pos.dim() == 2 or (bev_pos.dim() == 3 and bev_pos.shape[0] in (1, B))), "bev_pos: ([1 or B,] H*W, 2) float32"
    assert enc_weight.dtype == torch.float32 and enc_weight.numel() == Fd * num_classes and tuple(enc_weight.shape[:2]) == (Fd, num_classes), \
        "enc_weight: (F, C[, 1]) float32"
    assert enc_bias.dtype == torch.float32 and tuple(enc_bias.shape) == (Fd,), "enc_bias: (F,) float32"
    assert top_class.dtype == torch.int64 and top_index.dtype == torch.int64 and top_class.dim() == 2 and \
        top_class.shape == top_index.shape and top_class.shape[0] == B and top_class.shape[1] >= 1, "top_class, top_index: (B, K) int64"


class BoxDecoder:
    """post_processing_cfg: the head's POST_PROCESSING (SCORE_THRESH, POST_CENTER_RANGE, SCORE_THRESH_UNK or none);
    feature_map_stride, voxel_size, point_cloud_range as the head holds them; unknown_labels: the 1-based labels of
    pseudo_processor.unknown_labels (() without one); relabel_map: the head's relabel_map (C + 1 entries, indexed by the
    1-based label) when relabel_classes is on.

    decode_padded(preds, query_labels) -> boxes (B, K, 7 or 9), scores (B, K), labels (B, K) int32 and counts (B) int32 on the
    device, each scene's kept rows first and in query order, zeros behind; no synchronisation.
    get_bboxes(preds, query_labels) -> the reference's list of {'pred_boxes', 'pred_scores', 'pred_labels'}; reads the counts
    once on the host (the reference's boolean indexing synchronises there as well).  preds: 'heatmap' (B, C, K) logits,
    'query_heatmap_score', 'center', 'height', 'dim', 'rot' and optionally 'vel'; it is not modified (the reference's decode
    overwrites center in place)."""

    def __init__(self, post_processing_cfg, feature_map_stride, voxel_size, point_cloud_range, num_classes, unknown_labels=(),
                 relabel_map=None):
        self.num_classes = int(num_classes)
        assert 1 <= self.num_classes <= 64, "the unknown labels cross the ABI as a 64-bit mask: 1 <= num_classes <= 64"
        self.score_thresh = float(_get(post_processing_cfg, "SCORE_THRESH"))
        unk = _get(post_processing_cfg, "SCORE_THRESH_UNK", None)
        self.score_thresh_unk = self.score_thresh if unk is None else float(unk)
        rng = [float(v) for v in _get(post_processing_cfg, "POST_CENTER_RANGE")]
        assert len(rng) == 6, "POST_CENTER_RANGE has 6 entries"
        self.post_center_range = rng
        self._range_c = (ctypes.c_float * 6)(*rng)
        self.stride = int(feature_map_stride)
        self.voxel = [float(v) for v in list(voxel_size)[:2]]
        self.origin = [float(v) for v in list(point_cloud_range)[:2]]
        self.unk_mask = 0
        if unk is not None:
            for label in unknown_labels:
                if 1 <= int(label) <= self.num_classes:
                    self.unk_mask |= 1 << (int(label) - 1)
        self.relabel_map = None
        if relabel_map is not None:
            table = [int(relabel_map[i]) for i in range(self.num_classes + 1)]
            self.relabel_map = torch.tensor(table, dtype=torch.int32)
        self._relabel_dev = {}

    def _relabel(self, dev):
        if self.relabel_map is None:
            return None
        if dev not in self._relabel_dev:
            self._relabel_dev[dev] = self.relabel_map.to(dev)
        return self._relabel_dev[dev]

    def check(self, preds, query_labels):
        """host-side argument checks (no library needed) -> B, K, has_vel"""
        hm = preds["heatmap"]
        assert hm.dim() == 3 and hm.shape[1] == self.num_classes, f"heatmap: (B, {self.num_classes}, K)"
        B, C, K = (int(s) for s in hm.shape)
        want = {"heatmap": C, "query_heatmap_score": C, "center": 2, "height": 1, "dim": 3, "rot": 2}
        if preds.get("vel") is not None:
            want["vel"] = 2
        for key, n in want.items():
            t = preds[key]
            assert t.dtype == torch.float32, f"{key} must be float32, got {t.dtype}"
            assert tuple(t.shape) == (B, n, K), f"{key}: expected {(B, n, K)}, got {tuple(t.shape)}"
        assert query_labels.dtype == torch.int64 and tuple(query_labels.shape) == (B, K), "query_labels: (B, K) int64"
        assert K >= 1
        return B, K, "vel" in want

    def decode_padded(self, preds, query_labels):
        B, K, has_vel = self.check(preds, query_labels)
        L = lib.load()
        t = {k: preds[k].detach().contiguous() for k in ("heatmap", "query_heatmap_score", "center", "height", "dim", "rot")}
        vel = preds["vel"].detach().contiguous() if has_vel else None
        lib.require_device(query_labels, vel, *t.values())
        dev = t["heatmap"].device
        boxes = torch.empty((B, K, 9 if has_vel else 7), dtype=torch.float32, device=dev)
        scores = torch.empty((B, K), dtype=torch.float32, device=dev)
        labels = torch.empty((B, K), dtype=torch.int32, device=dev)
        counts = torch.empty((B,), dtype=torch.int32, device=dev)
        if B:
            lib.check(L.fnp_tf_decode(lib.ptr(t["heatmap"]), lib.ptr(t["query_heatmap_score"]), lib.ptr(t["center"]), lib.ptr(t["height"]),
                                      lib.ptr(t["dim"]), lib.ptr(t["rot"]), lib.ptr(vel), lib.ptr(query_labels.contiguous()), B,
                                      self.num_classes, K, self.stride, self.voxel[0], self.voxel[1], self.origin[0], self.origin[1],
                                      self.score_thresh, self.score_thresh_unk, self.unk_mask, self._range_c,
                                      lib.ptr(self._relabel(dev)), lib.ptr(boxes), lib.ptr(scores), lib.ptr(labels), lib.ptr(counts),
                                      lib.stream()), "fnp_tf_decode")
        return boxes, scores, labels, counts

    def get_bboxes(self, preds, query_labels, pseudo_nms_thresh=None):
        """pseudo_nms_thresh: the training-only PSEUDO_NMS_THRESH branch, run on the compacted rows with nms_normal_gpu"""
        boxes, scores, labels, counts = self.decode_padded(preds, query_labels)
        out = []
        for b, n in enumerate(counts.tolist()):
            d = {"pred_boxes": boxes[b, :n], "pred_scores": scores[b, :n], "pred_labels": labels[b, :n]}
            if n and pseudo_nms_thresh:
                from ..iou3d_nms import iou3d_nms_utils

                keep, _ = iou3d_nms_utils.nms_normal_gpu(d["pred_boxes"][:, :7], d["pred_scores"], thresh=pseudo_nms_thresh)
                d = {k: v[keep] for k, v in d.items()}
            out.append(d)
        return out


# ---- plain-torch mirrors of the same spans ----------------------------------------------------------------------------------


def proposals_plain(dense_heatmap, num_proposals, point_class_list, from_logits=True, stable=True):
    """predict :201-294 and :321-324 as torch ops on dense_heatmap's device.  stable=True sorts with the library's tie rule
    (value descending, flat index ascending); stable=False is the reference's argsort."""
    heatmap = dense_heatmap.detach().sigmoid() if from_logits else dense_heatmap.detach()
    B, C, H, W = heatmap.shape
    local_max = torch.zeros_like(heatmap)
    local_max[:, :, 1:-1, 1:-1] = F.max_pool2d(heatmap, kernel_size=3, stride=1, padding=0)
    for c in point_class_list:
        local_max[:, c] = heatmap[:, c]
    heatmap = heatmap * (heatmap == local_max)
    heatmap = heatmap.view(B, C, -1)
    flat = heatmap.view(B, -1)
    if stable:
        order = torch.sort(flat, dim=-1, descending=True, stable=True).indices[..., :num_proposals]
    else:
        order = flat.argsort(dim=-1, descending=True)[..., :num_proposals]
    top_class = order // heatmap.shape[-1]
    top_index = order % heatmap.shape[-1]
    top_score = flat.gather(1, order)
    qhs = heatmap.gather(index=top_index[:, None, :].expand(-1, C, -1), dim=-1)
    return top_class, top_index, top_score, qhs


def init_queries_plain(lidar_feat_flatten, bev_pos, enc_weight, enc_bias, top_class, top_index):
    """predict :295-313 as torch ops; differentiable in the features, the class encoding and the positions"""
    B, Fd, HW = lidar_feat_flatten.shape
    C = enc_weight.shape[1]
    query_feat = lidar_feat_flatten.gather(index=top_index[:, None, :].expand(-1, Fd, -1), dim=-1)
    one_hot = F.one_hot(top_class, num_classes=C).permute(0, 2, 1)
    query_feat = query_feat + F.conv1d(one_hot.float(), enc_weight.reshape(Fd, C, 1), enc_bias)
    pos = bev_pos if bev_pos.dim() == 3 else bev_pos[None]
    pos = pos.expand(B, -1, -1)
    query_pos = pos.gather(index=top_index[:, :, None].expand(-1, -1, 2), dim=1).flip(dims=[-1])
    return query_feat, query_pos


def get_bboxes_plain(preds, query_labels, decoder):
    """get_bboxes + decode_bbox(filter=True) (:616-728) as torch ops with `decoder`'s (a BoxDecoder's) settings, the Python loop
    over queries included.  preds is not modified."""
    C = decoder.num_classes
    heat = preds["heatmap"].sigmoid()
    one_hot = F.one_hot(query_labels, num_classes=C).permute(0, 2, 1)
    heat = heat * preds["query_heatmap_score"] * one_hot
    center, height, dim, rot, vel = preds["center"].clone(), preds["height"], preds["dim"], preds["rot"], preds.get("vel")
    post_center_range = torch.tensor(decoder.post_center_range, device=heat.device).float()
    final_preds = heat.max(1, keepdims=False).indices
    final_scores = heat.max(1, keepdims=False).values
    unknown = [l for l in range(1, C + 1) if (decoder.unk_mask >> (l - 1)) & 1]
    is_unknown = torch.zeros_like(final_preds, dtype=torch.float)
    for b, batch_preds in enumerate(final_preds):
        for idx, label in enumerate(batch_preds):
            label = label.item() + 1
            is_unknown[b, idx] = float(label in unknown)
    center[:, 0, :] = center[:, 0, :] * decoder.stride * decoder.voxel[0] + decoder.origin[0]
    center[:, 1, :] = center[:, 1, :] * decoder.stride * decoder.voxel[1] + decoder.origin[1]
    dim = dim.exp()
    rot = torch.atan2(rot[:, 0:1, :], rot[:, 1:2, :])
    parts = [center, height, dim, rot] + ([vel] if vel is not None else [])
    final_box_preds = torch.cat(parts, dim=1).permute(0, 2, 1)
    score_threshs = decoder.score_thresh * (1 - is_unknown) + is_unknown * decoder.score_thresh_unk
    mask = final_scores > score_threshs
    mask &= (final_box_preds[..., :3] >= post_center_range[:3]).all(2)
    mask &= (final_box_preds[..., :3] <= post_center_range[3:]).all(2)
    out = []
    for i in range(heat.shape[0]):
        labels = final_preds[i, mask[i]].int() + 1
        if decoder.relabel_map is not None:
            for j in range(labels.numel()):
                labels[j] = int(decoder.relabel_map[labels[j].item()])
        out.append({"pred_boxes": final_box_preds[i, mask[i]], "pred_scores": final_scores[i, mask[i]], "pred_labels": labels})
    return out
