#!/usr/bin/env python3
"""TransFusion head, Hungarian assignment and per-query targets: the device span (dense_heads.transfusion_assign.QueryTargets,
four launches of csrc/tfassign.hip for the batch) against the library's plain route on the same card, in the same
process, alternating.  One JSON line.

workload  K = 200 queries, C = 10, B in {1, 4} scenes, M in {10, 40, 100} valid boxes per scene in a capacity of Mcap = M + 12,
          padding rows between them.  Seeded head outputs that put a query near most boxes, as the heatmap proposals do.
plain     the library's plain route, query_targets_plain: per scene, plain torch on the device with the library's
          fnp_boxes_overlap_bev for the BEV term, one read of the valid rows, the cost to the host, fnp_host_lsap there, the
          match back, the indexed target writes.  It reads back twice per scene; the reference itself reads once per
          ground-truth row on top of that, so the reference is slower than this span, not faster.
timing    kernels: HIP events around `--inner` back-to-back launches of ONE entry point on the buffers a complete call left
          (raw ctypes calls), median (p10, p90) over `--reps` groups after warm-up; fnp_tf_assign_cost is its two launches.
          spans: a host clock around one call that ends in a device synchronise (the plain span's time is host time: it
          synchronises twice per scene), the two spans alternating.  scipy alone on the host matrix is timed too.
losses    query_loss forward + backward (three launches) against query_loss_plain under autograd, the same host clock.
check     both spans give the same assignment on every workload before anything is timed.

    python tools/bench_assign.py [--reps 30] [--inner 20]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from findnpropagate_amd import lib  # noqa: E402
from findnpropagate_amd.dense_heads.transfusion_assign import QueryTargets, query_targets_plain  # noqa: E402
from findnpropagate_amd.utils.loss_utils import query_loss, query_loss_plain  # noqa: E402

K, C, STRIDE, VOXEL, RANGE = 200, 10, 8, (0.075, 0.075, 0.2), (-54.0, -54.0, -5.0, 54.0, 54.0, 3.0)
W_CLS, ALPHA, EPS, W_REG, W_IOU = 0.15, 0.25, 1e-12, 0.25, 0.25


def make_inputs(rng, B, M, Mcap):
    gt = np.zeros((B, Mcap, 10), np.float32)
    preds = {h: np.zeros((B, n, K), np.float32) for h, n in (("heatmap", C), ("center", 2), ("height", 1), ("dim", 3), ("rot", 2), ("vel", 2))}
    for b in range(B):
        box = np.zeros((M, 10))
        box[:, 0:2], box[:, 2] = rng.uniform(-50, 50, (M, 2)), rng.uniform(-2.5, 0.5, M)
        box[:, 3:6], box[:, 6] = np.exp(rng.uniform(np.log(0.6), np.log(6.0), (M, 3))), rng.uniform(-np.pi, np.pi, M)
        box[:, 7:9], box[:, 9] = rng.normal(0, 2, (M, 2)), rng.integers(1, C + 1, M)
        gt[b, np.sort(rng.choice(Mcap, M, replace=False))] = box
        xy, z, dims, yaw = rng.uniform(-52, 52, (K, 2)), rng.uniform(-3, 1, K), rng.uniform(-0.7, 2.0, (K, 3)), rng.uniform(-np.pi, np.pi, K)
        logit = rng.normal(-2.5, 1.2, (C, K))
        near = rng.permutation(K)[:M]
        xy[near], z[near] = box[:, 0:2] + rng.normal(0, 0.5, (M, 2)), box[:, 2] + rng.normal(0, 0.2, M)
        dims[near], yaw[near] = np.log(box[:, 3:6]) + rng.normal(0, 0.15, (M, 3)), box[:, 6] + rng.normal(0, 0.2, M)
        logit[box[:, 9].astype(int) - 1, near] += rng.uniform(1.0, 4.0, M)
        preds["heatmap"][b], preds["height"][b, 0], preds["dim"][b] = logit, z, dims.T
        preds["center"][b] = ((xy - np.array(RANGE[0:2])) / (STRIDE * np.array(VOXEL[0:2]))).T
        preds["rot"][b, 0], preds["rot"][b, 1] = np.sin(yaw), np.cos(yaw)
        preds["vel"][b] = rng.normal(0, 2, (2, K))
    return preds, gt


def plain_span(qt, preds, gt):
    """the library's plain route (dense_heads.transfusion_assign.query_targets_plain) -> assigned, bbox_targets"""
    o = query_targets_plain(qt, preds, gt)
    return o["assigned"], o["bbox_targets"]


def stats(ts):
    ts = np.sort(ts)
    return round(float(np.median(ts)), 1), round(float(ts[len(ts) // 10]), 1), round(float(ts[-1 - len(ts) // 10]), 1)


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def event_timed(fn, inner):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    z.record()
    z.synchronize()
    return a.elapsed_time(z) * 1e3 / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_assign.py measures on the GPU; there is no other route"
    L = lib.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2)
    qt = QueryTargets(dict(FEATURE_MAP_STRIDE=STRIDE), RANGE, VOXEL, C)
    rows = []
    for B in (1, 4):
        for M in (10, 40, 100):
            Mcap = M + 12
            preds, gt = make_inputs(rng, B, M, Mcap)
            preds, gt = {h: torch.from_numpy(v).to(dev) for h, v in preds.items()}, torch.from_numpy(gt).to(dev)
            o = qt(preds, gt, return_debug=True)
            want, want_t = plain_span(qt, preds, gt)
            assert torch.equal(o["assigned"], want), "device assignment differs from the plain span's"
            assert torch.allclose(o["bbox_targets"], want_t, rtol=1e-5, atol=1e-6)
            host_cost = o["cost"].cpu().numpy()
            s, P = lib.stream(), lib.ptr
            heads = [P(preds[h]) for h in ("heatmap", "center", "height", "dim", "rot", "vel")]
            rng6 = (ctypes.c_float * 6)(*qt.range)
            scratch = {k: torch.empty_like(v) for k, v in o.items()}
            unk = torch.empty((B, K), dtype=torch.uint8, device=dev)
            kernels = {
                "cost_2_launches": lambda: L.fnp_tf_assign_cost(*heads, P(gt), B, C, K, Mcap, 10, STRIDE, VOXEL[0], VOXEL[1], rng6, W_CLS, ALPHA, 2.0,
                                                                EPS, W_REG, W_IOU, P(scratch["num_valid"]), P(scratch["valid_map"]),
                                                                P(scratch["cost"]), P(scratch["iou"]), P(scratch["boxes"]), s),
                "match": lambda: L.fnp_tf_assign_match(P(o["cost"]), P(o["iou"]), P(o["num_valid"]), P(o["valid_map"]), B, K, Mcap,
                                                       P(scratch["assigned"]), P(scratch["matched_ious"]), s),
                "target": lambda: L.fnp_tf_assign_targets(P(o["assigned"]), P(gt), B, C, K, Mcap, 10, STRIDE, VOXEL[0], VOXEL[1], qt.range[0],
                                                          qt.range[1], 0, P(scratch["labels"]), P(scratch["label_weights"]),
                                                          P(scratch["bbox_targets"]), P(scratch["bbox_weights"]), P(unk), P(scratch["num_pos"]), s),
            }
            for _ in range(5):
                qt(preds, gt), plain_span(qt, preds, gt)
                for fn in kernels.values():
                    assert fn() == 0
            lcfg = dict(LOSS_WEIGHTS=dict(code_weights=[1.0] * 8 + [0.2, 0.2]))
            order = ["center", "height", "dim", "rot", "vel"]
            grad_preds = {h: v.clone().requires_grad_(True) for h, v in preds.items()}

            def loss_step(fn):
                a, b = fn(grad_preds, o, lcfg, order)
                (a + b).backward()

            for _ in range(5):
                loss_step(query_loss), loss_step(query_loss_plain)
            t = {k: [] for k in (*kernels, "device_span", "plain_span", "scipy_alone", "loss_fwd_bwd_device", "loss_fwd_bwd_plain")}
            for _ in range(args.reps):
                for k, fn in kernels.items():
                    t[k].append(event_timed(fn, args.inner))
                t["device_span"].append(host_timed(lambda: qt(preds, gt)))
                t["plain_span"].append(host_timed(lambda: plain_span(qt, preds, gt)))
                t["loss_fwd_bwd_device"].append(host_timed(lambda: loss_step(query_loss)))
                t["loss_fwd_bwd_plain"].append(host_timed(lambda: loss_step(query_loss_plain)))
                t0 = time.perf_counter()
                for b in range(B):
                    linear_sum_assignment(host_cost[b, :, :M])
                t["scipy_alone"].append((time.perf_counter() - t0) * 1e6)
            row = {"B": B, "M": M, **{k + "_us": stats(v) for k, v in t.items()}}
            row["plain_over_device"] = round(row["plain_span_us"][0] / row["device_span_us"][0], 1)
            rows.append(row)
    print(json.dumps({"bench": "assign", "K": K, "C": C, "units": "us, median (p10, p90)", "reps": args.reps, "inner": args.inner,
                      "device": torch.cuda.get_device_name(0), "rows": rows}))


if __name__ == "__main__":
    main()
