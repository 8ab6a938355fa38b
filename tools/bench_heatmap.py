#!/usr/bin/env python3
"""TransFusion heatmap targets + heatmap loss (forward and backward): the device path against this repository's plain mirrors on
the same card.  One JSON line.

workload  4 scenes with 50, 150 and 400 boxes each on the shipped 180 x 180 x 10 map (sides log-uniform 0.5 .. 12 m), f32 logits.
fused     dense_heads.transfusion_targets.HeatmapTargets + utils.loss_utils.heatmap_loss + backward: six kernels, no host read.
          HIP events around `--inner` back-to-back repetitions, median over `--reps` such groups after warm-up; the three parts
          (targets, loss forward, loss backward) also on their own, with the bytes they must move: targets write the map once
          (B C H W x 4 B), the loss forward reads logits and targets once (8 B per element), the backward reads both and writes
          the gradient (12 B per element).
plain     the reference's structure with model_utils.centernet_utils / utils.loss_utils on the same device: the Python loop
          over boxes of transfusion_head.py:451-470 (gaussian_radius on one-element tensors, a numpy Gaussian uploaded per box,
          device-to-host reads), then GaussianFocalLoss(clip_sigmoid(x)).sum() / max(heatmap.eq(1).float().sum().item(), 1) and
          backward.  It synchronises by itself; wall clock closed by a device synchronisation, median of `--plain-reps`.

    python tools/bench_heatmap.py [--reps 30] [--inner 20] [--plain-reps 5] [--boxes 50 150 400]

Kernel times (the event times above are launch-bound: six small kernels and their Python): a run of its own under
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_heatmap.py --plain-reps 0 --boxes 400
and the hm_* rows of DIR's kernel_stats.csv.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from findnpropagate_amd.dense_heads.transfusion_targets import HeatmapTargets  # noqa: E402
from findnpropagate_amd.model_utils import centernet_utils  # noqa: E402
from findnpropagate_amd.model_utils.transfusion_utils import clip_sigmoid  # noqa: E402
from findnpropagate_amd.utils.loss_utils import GaussianFocalLoss, heatmap_loss  # noqa: E402

CFG = {"FEATURE_MAP_STRIDE": 8, "GAUSSIAN_OVERLAP": 0.1, "MIN_RADIUS": 2, "UNK_RADIUS_MULT": 1}
GRID, PCR, VOXEL, C = [1440, 1440, 40], [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], [0.075, 0.075, 0.2], 10


def scenes(rng, B, M):
    b = np.zeros((B, M, 10), np.float32)
    b[..., 0:2] = rng.uniform(-54, 54, (B, M, 2))
    b[..., 3:6] = np.exp(rng.uniform(np.log(0.5), np.log(12.0), (B, M, 3)))
    b[..., 9] = rng.integers(1, C + 1, (B, M))
    return b


def events(fn, reps, inner, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        z.record()
        z.synchronize()
        ts.append(a.elapsed_time(z) * 1e3 / inner)
    ts = np.sort(ts)
    return round(float(np.median(ts)), 2), round(float(ts[len(ts) // 10]), 2), round(float(ts[-1 - len(ts) // 10]), 2)


def plain_targets(gt_boxes, H, W):
    """transfusion_head.py:352-375 and :446-470 with the plain mirrors, on gt_boxes' device"""
    maps = []
    for scene in gt_boxes:
        boxes, labels = scene[:, :-1], scene[:, -1].long() - 1
        heatmap = boxes.new_zeros(C, H, W)
        for idx in range(len(boxes)):
            width = boxes[idx][3] / VOXEL[0] / CFG["FEATURE_MAP_STRIDE"]
            length = boxes[idx][4] / VOXEL[1] / CFG["FEATURE_MAP_STRIDE"]
            if width > 0 and length > 0:
                radius = centernet_utils.gaussian_radius(length.view(-1), width.view(-1), CFG["GAUSSIAN_OVERLAP"])[0]
                radius = max(CFG["MIN_RADIUS"], int(radius))
                coor_x = (boxes[idx][0] - PCR[0]) / VOXEL[0] / CFG["FEATURE_MAP_STRIDE"]
                coor_y = (boxes[idx][1] - PCR[1]) / VOXEL[1] / CFG["FEATURE_MAP_STRIDE"]
                center_int = torch.tensor([coor_x, coor_y], dtype=torch.float32, device=boxes.device).to(torch.int32)
                centernet_utils.draw_gaussian_to_heatmap(heatmap[labels[idx]], center_int, radius)
        maps.append(heatmap)
    return torch.stack(maps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--plain-reps", type=int, default=5)
    ap.add_argument("--boxes", type=int, nargs="*", default=[50, 150, 400])
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    head = HeatmapTargets(CFG, GRID, PCR, VOXEL, C)
    B, H, W = 4, head.H, head.W
    n = B * C * H * W
    logits = torch.from_numpy(rng.normal(-2, 3, (B, C, H, W)).astype(np.float32)).to(dev).requires_grad_(True)
    loss_fn = GaussianFocalLoss()
    out = {"metric": "heatmap_targets_and_loss", "scenes": B, "map": [C, H, W], "elements": n}
    for M in a.boxes:
        gt = torch.from_numpy(scenes(rng, B, M)).to(dev)
        hm_buf = torch.empty((B, C, H, W), device=dev)

        def fused():
            logits.grad = None
            hm, num_pos = head(gt, out=hm_buf)
            heatmap_loss(logits, hm, num_pos).backward()

        def plain():
            logits.grad = None
            hm = plain_targets(gt, H, W)
            loss = loss_fn(clip_sigmoid(logits.clone()), hm).sum() / max(hm.eq(1).float().sum().item(), 1)
            loss.backward()
            return hm, loss

        hm, num_pos = head(gt, out=hm_buf)
        ref_hm, ref_loss = plain()
        res = {"boxes_per_scene": M, "maps_equal_on_device": bool(torch.equal(hm, ref_hm)), "num_pos": int(num_pos.item())}
        med, lo, hi = events(fused, a.reps, a.inner)
        res.update(fused_us=med, fused_p10_us=lo, fused_p90_us=hi)
        med, lo, hi = events(lambda: head(gt, out=hm_buf), a.reps, a.inner)
        res.update(targets_us=med, targets_p10_us=lo, targets_p90_us=hi, targets_write_GBps=round(4 * n / med / 1e3, 1))
        loss = heatmap_loss(logits, hm, num_pos)
        med, lo, hi = events(lambda: heatmap_loss(logits, hm, num_pos), a.reps, a.inner)
        res.update(loss_forward_us=med, loss_forward_p10_us=lo, loss_forward_p90_us=hi, loss_forward_GBps=round(8 * n / med / 1e3, 1))
        one = torch.ones((), device=dev)
        med, lo, hi = events(lambda: torch.autograd.grad(loss, logits, one, retain_graph=True), a.reps, a.inner)
        res.update(loss_backward_us=med, loss_backward_p10_us=lo, loss_backward_p90_us=hi, loss_backward_GBps=round(12 * n / med / 1e3, 1))
        if not a.plain_reps:          # (a profiling run: the fused kernels only)
            out[f"m{M}"] = res
            continue
        ts = []
        for _ in range(a.plain_reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            plain()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
        res.update(plain_ms=round(float(np.median(ts)), 2), plain_over_fused=round(float(np.median(ts)) * 1e3 / res["fused_us"], 1))
        # the plain loss alone (forward + backward, the targets given): what the fused loss replaces
        def plain_loss():
            logits.grad = None
            (loss_fn(clip_sigmoid(logits.clone()), hm).sum() / max(hm.eq(1).float().sum().item(), 1)).backward()
        ts = []
        for _ in range(max(a.plain_reps, 20)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            plain_loss()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
        res.update(plain_loss_ms=round(float(np.median(ts)), 3), fused_loss_rel_diff=abs(float(loss.item()) - float(ref_loss.item())) / abs(float(ref_loss.item())))
        out[f"m{M}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
