#!/usr/bin/env python3
"""Golden vectors for the Hungarian assignment and the per-query targets of TransFusionHead by RUNNING THE REFERENCE on the
CPU: pcdet/models/dense_heads/transfusion_head.py (TransFusionHead.get_targets, get_targets_single, decode_bbox and
encode_bbox, called unbound on a stand-in self) with the reference's real HungarianAssigner3D
(target_assigner/hungarian_assigner.py) and real scipy.

Two things are neutralised for the run: Tensor.cuda returns self, and iou3d_nms_cuda.boxes_overlap_bev_gpu is a stub that fills
its output from the library's host function fnp_host_boxes_overlap_bev.  THE BEV OVERLAP IN THIS FIXTURE IS THEREFORE THE
LIBRARY'S HOST FUNCTION, not the reference's kernel; its device twin is held to the reference's own kernel by
tests/test_gpu_box_at_scale.py.  The dense heatmap the method also returns is not recorded (tests/golden/heatmap_golden.npz
holds that slice).  The two query losses and their gradients in every head output come from TransFusionHead.loss run the same
way, once on f32 and once on f64 copies of the inputs.

Runs in the build container only (needs the reference and the built library).  Per case (tests/ref_assign.py CASES) it records
the inputs, the decoded boxes, per scene the cost matrix as scipy received it with the IoU matrix and the match, and
get_targets' outputs.  A condition on the cases, checked here: for every scene scipy's match is the same on the reference's
f32 cost, on the f64 evaluation of the cost, and on 32 copies of the f32 cost with every entry moved by a random sign times
the cost bound of ref_assign.py; a scene that fails makes the case be drawn again from the next seed.  That shows the cases
are well separated; it is no tolerance on a kernel.  Output: tests/golden/assign_golden.npz (arrays only)."""
import functools
import importlib
import os
import sys
import types

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_assign as R  # noqa: E402
from make_heatmap_golden import AttrDict, REF, shell, stub  # noqa: E402
from findnpropagate_amd import lib  # noqa: E402


def host_overlap_bev(a, b, out):
    a, b = a.float().contiguous(), b.float().contiguous()
    tmp = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.float32)
    lib.check(lib.load().fnp_host_boxes_overlap_bev(lib.ptr(a), a.shape[0], lib.ptr(b), b.shape[0], lib.ptr(tmp)), "overlap")
    out.copy_(tmp)


def load_reference():
    class _Any:
        def __getattr__(self, k):
            return _Any()

        def __call__(self, *a, **k):
            return _Any()

    for name in ("SharedArray", "cv2", "easydict", "spconv", "spconv.pytorch", "cumm", "cumm.tensorview", "numba", "tqdm",
                 "matplotlib", "matplotlib.pyplot", "torchvision", "torchvision.utils", "torchvision.ops"):
        stub(name).__getattr__ = lambda k: _Any()  # type: ignore
    p = os.path.join(REF, "pcdet")
    shell("pcdet", p)
    shell("pcdet.utils", os.path.join(p, "utils"))
    shell("pcdet.ops", os.path.join(p, "ops"))
    ops = shell("pcdet.ops.iou3d_nms", os.path.join(p, "ops", "iou3d_nms"))
    ops.iou3d_nms_utils = stub("pcdet.ops.iou3d_nms.iou3d_nms_utils")
    ops.iou3d_nms_cuda = stub("pcdet.ops.iou3d_nms.iou3d_nms_cuda", boxes_overlap_bev_gpu=host_overlap_bev)
    shell("pcdet.models", os.path.join(p, "models"))
    shell("pcdet.models.dense_heads", os.path.join(p, "models", "dense_heads"))
    shell("pcdet.models.model_utils", os.path.join(p, "models", "model_utils"))
    shell("pcdet.models.dense_heads.target_assigner", os.path.join(p, "models", "dense_heads", "target_assigner"))
    stub("pcdet.models.dense_heads.pseudo_processor", PseudoProcessor=object)
    stub("pcdet.models.model_utils.basic_block_2d", BasicBlock2D=object)
    stub("pcdet.utils.box_utils")
    ha = importlib.import_module("pcdet.models.dense_heads.target_assigner.hungarian_assigner")
    th = importlib.import_module("pcdet.models.dense_heads.transfusion_head")
    return th, ha


def stand_in(th, ha, cfg):
    """the attributes get_targets and the methods behind it read from self"""
    H = th.TransFusionHead
    s = types.SimpleNamespace()
    for m in ("get_targets_single", "decode_bbox", "encode_bbox"):
        setattr(s, m, functools.partial(getattr(H, m), s))
    s.bbox_assigner = ha.HungarianAssigner3D(**R.ASSIGNER)
    s.code_size, s.num_classes = cfg["code"], cfg["C"]
    s.use_pseudo = bool(cfg["unknown_labels"])
    s.pseudo_processor = types.SimpleNamespace(unknown_labels=list(cfg["unknown_labels"]))
    s.model_cfg = AttrDict(TARGET_ASSIGNER_CONFIG=AttrDict(GAUSSIAN_OVERLAP=0.1, MIN_RADIUS=2, UNK_RADIUS_MULT=1),
                           POST_PROCESSING=AttrDict(SCORE_THRESH=0.0, POST_CENTER_RANGE=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]))
    s.grid_size = np.array([1440, 1440, 40])        # (the dense heatmap is drawn and dropped, not recorded)
    s.feature_map_stride = R.STRIDE
    s.voxel_size = list(R.VOXEL)
    s.point_cloud_range = list(R.RANGE)
    return s


def run_case(th, ha, name, seed):
    cfg = R.CASES[name]
    preds, gt = R.case_inputs(name, seed)
    seen = []
    real = ha.linear_sum_assignment

    def recorder(cost):
        r, c = real(cost)
        seen.append((cost.numpy().copy(), r.copy(), c.copy()))
        return r, c

    ious = []
    real_iou = ha.HungarianAssigner3D.iou3d_cost

    def iou_recorder(self, *a):
        out = real_iou(self, *a)
        ious.append(out[1].numpy().copy())
        return out

    boxes = []
    real_decode = th.TransFusionHead.decode_bbox

    def decode_recorder(self, *a, **k):
        out = real_decode(self, *a, **k)
        boxes.append(out[0]["pred_boxes"].numpy().copy())
        return out

    s = stand_in(th, ha, cfg)
    s.decode_bbox = functools.partial(decode_recorder, s)
    ha.linear_sum_assignment, ha.HungarianAssigner3D.iou3d_cost = recorder, iou_recorder
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        t = torch.from_numpy(gt)
        out = th.TransFusionHead.get_targets(s, t[..., :-1], t[..., -1].long() - 1, {k: torch.from_numpy(v) for k, v in preds.items()})
    finally:
        ha.linear_sum_assignment, ha.HungarianAssigner3D.iou3d_cost, torch.Tensor.cuda = real, real_iou, cuda
    labels, label_weights, bbox_targets, bbox_weights, num_pos, matched_ious, _, unknown_mask = out
    save = {"gt_boxes": gt, "boxes": np.stack(boxes), "labels": labels.numpy(), "label_weights": label_weights.numpy(),
            "bbox_targets": bbox_targets.numpy(), "bbox_weights": bbox_weights.numpy(), "num_pos": np.int64(num_pos),
            "matched_ious": matched_ious.numpy(), "unknown_mask": unknown_mask.numpy(), "seed": np.int64(seed)}
    save.update({"pred_" + k: v for k, v in preds.items()})
    # scipy saw one matrix per scene that has valid rows, in scene order
    it, it_iou = iter(seen), iter(ious)
    separated = True
    for b in range(gt.shape[0]):
        rows = R.valid_rows(gt[b], cfg["C"])
        if rows.size == 0:
            continue
        cost, r, c = next(it)
        iou = next(it_iou)
        assert cost.shape == (cfg["K"], rows.size)
        save[f"cost{b}"], save[f"iou{b}"], save[f"match_rows{b}"], save[f"match_cols{b}"] = cost, iou, r, c
        separated &= well_separated(preds, gt, b, rows, cost, iou, c, seed)
    assert next(it, None) is None
    return save, separated


def run_loss(th, ha, name, seed, dtype):
    """TransFusionHead.loss unbound on the stand-in, with the reference's real SigmoidFocalClassificationLoss and L1Loss, on the
    case's inputs as `dtype` -> loss_cls, loss_bbox and the gradient of their sum in every head output.  hm_weight is 0 and
    cls_weight = bbox_weight = 1, so the heatmap head's gradient is loss_cls's alone and the other heads' loss_bbox's."""
    cfg = R.CASES[name]
    preds, gt = R.case_inputs(name, seed)
    s = stand_in(th, ha, cfg)
    lu = th.loss_utils
    names = [f"c{i}" for i in range(cfg["C"])]
    s.class_names = names
    s.pseudo_processor.all_class_names = names
    s.pseudo_processor.forward_pseudo_stats = {f"num_per_class_{n}": 0 for n in names}
    seen = []

    def get_targets(*a):
        seen.append(th.TransFusionHead.get_targets(s, *a))
        return seen[-1]

    s.get_targets = get_targets
    s.loss_heatmap, s.loss_cls, s.loss_bbox = lu.GaussianFocalLoss(), lu.SigmoidFocalClassificationLoss(gamma=2.0, alpha=0.25), lu.L1Loss()
    s.loss_heatmap_weight, s.loss_cls_weight, s.loss_bbox_weight = 0.0, 1.0, 1.0
    s.label_smoothing, s.balanced_reweighting = False, False
    s.model_cfg["LOSS_CONFIG"] = AttrDict(LOSS_WEIGHTS=R.loss_weights(name))
    s.model_cfg["SEPARATE_HEAD_CFG"] = AttrDict(HEAD_ORDER=R.head_order(name))
    t = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in preds.items()}
    t["dense_heatmap"] = torch.zeros((gt.shape[0], cfg["C"], 180, 180), dtype=dtype)
    g = torch.from_numpy(gt).to(dtype)
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        total, log = th.TransFusionHead.loss(s, g[..., :-1], g[..., -1].long() - 1, t)
    finally:
        torch.Tensor.cuda = cuda
    total.backward()
    out = {"loss_cls": np.float64(log["loss_cls"]), "loss_bbox": np.float64(log["loss_bbox"])}
    out.update({"grad_" + k: t[k].grad.numpy() for k in preds})
    out["bbox_targets"] = seen[0][2].numpy()          # (the f64 run encodes from f64 logarithms: its targets differ in a last bit)
    return out


def well_separated(preds, gt, b, rows, cost32, iou32, cols, seed):
    box64, _ = R.decode_f64(preds, b)
    gts = gt[b, rows]
    clsreg, bound = R.cls_reg_f64(preds["heatmap"][b], box64, gts, gts[:, -1].astype(int) - 1)
    w = R.ASSIGNER["iou_cost"]["weight"]
    cost64 = clsreg - w * iou32.astype(np.float64)
    bev = torch.zeros(cost64.shape)
    host_overlap_bev(torch.from_numpy(box64[:, :7]), torch.from_numpy(gts[:, :7]), bev)
    bound = bound + w * R.iou_bound(box64, gts, bev.double().numpy(), R.decode_f64(preds, b)[1]) + R.U * np.abs(cost64)
    same = np.array_equal(linear_sum_assignment(cost64)[1], cols)
    rng = np.random.default_rng(seed + 1000 * b)
    for _ in range(32):
        moved = cost32.astype(np.float64) + rng.choice([-1.0, 1.0], cost32.shape) * bound
        same &= np.array_equal(linear_sum_assignment(moved.astype(np.float32))[1], cols)
    return bool(same)


def main():
    torch.set_num_threads(1)
    th, ha = load_reference()
    save = {}
    for name, cfg in R.CASES.items():
        for seed in range(cfg["seed"], cfg["seed"] + 20):
            arrays, ok = run_case(th, ha, name, seed)
            if ok:
                break
            print(name, "seed", seed, "is not well separated: drawn again")
        else:
            raise SystemExit(f"{name}: no well separated draw")
        assert seed == cfg["seed"], f"ref_assign.CASES['{name}']['seed'] must be {seed}"
        save.update({f"{name}_{k}": v for k, v in arrays.items()})
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            save.update({f"{name}_{tag}_{k}": v for k, v in run_loss(th, ha, name, seed, dt).items()})
        print(name, "loss_cls", save[f"{name}_f32_loss_cls"], save[f"{name}_f64_loss_cls"], "loss_bbox", save[f"{name}_f32_loss_bbox"], save[f"{name}_f64_loss_bbox"])
        print(name, "seed", seed, "num_pos", int(arrays["num_pos"]), "unknown", int(arrays["unknown_mask"].sum()))
    path = os.path.join(HERE, "assign_golden.npz")
    np.savez_compressed(path, **save)
    print(len(save), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
