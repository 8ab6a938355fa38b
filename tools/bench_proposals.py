#!/usr/bin/env python3
"""TransFusion head around its decoder: heatmap proposals (A), query initialisation (B) and box decode (C) on the device against
this repository's plain mirrors (dense_heads.transfusion_proposals.proposals_plain / init_queries_plain / get_bboxes_plain, the
reference's structure) on the same card, in the same process, interleaved.  One JSON line.

workload  the shipped 10 x 180 x 180 map, K = 200, 128 feature channels, f32 logits ~ N(-4, 2) (a sparse map after the sigmoid),
          at B = 1 and B = 4.  Decode inputs: seeded predictions with SCORE_THRESH 0.1.
device    A = three launches (header fill, mask + compaction + histogram, select + sort + scores), B = one, C = one: five
          launches end to end (read from the code, not from a trace); get_bboxes adds one device-to-host read of B counts.
          HIP events around `--inner` back-to-back repetitions, median over `--reps` groups after warm-up, for A, B and C on
          their own with the bytes each must move: A reads the map once (B C H W x 4 B), B reads and writes B F K x 4 B each
          way plus the indices, C reads 2 + 1 + 3 + 2 + 2 + 2 values per query and writes up to 9 + 2.
end to end  A + B + C, both paths, on a host clock closed by a device synchronisation (the plain decode synchronises by
          itself: an .item() per query), `--inner` repetitions per window, the two paths alternating window by window; the
          median over `--reps` windows.

    python tools/bench_proposals.py [--reps 20] [--inner 10] [--batches 1 4]
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

from findnpropagate_amd.dense_heads.transfusion_proposals import (BoxDecoder, HeatmapProposals, get_bboxes_plain,  # noqa: E402
                                                                  init_queries_plain, proposals_plain)

C, H, W, K, FEAT = 10, 180, 180, 200, 128
POST = {"SCORE_THRESH": 0.1, "POST_CENTER_RANGE": [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]}
STRIDE, VOXEL, PCR = 8, [0.075, 0.075, 0.2], [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
DEVICE_LAUNCHES = {"proposals": 3, "init_queries": 1, "decode": 1}


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


def wall(fn, inner):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6 / inner


def bev_pos_table(dev):
    xs, ys = torch.meshgrid(torch.linspace(0, W - 1, W), torch.linspace(0, H - 1, H), indexing="ij")
    return torch.stack([xs.reshape(-1) + 0.5, ys.reshape(-1) + 0.5], dim=1).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 4])
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    head = HeatmapProposals(K, 3, C, "nuScenes")
    dec = BoxDecoder(POST, STRIDE, VOXEL, PCR, C)
    pos = bev_pos_table(dev)
    enc_w = torch.from_numpy(rng.normal(0, 0.5, (FEAT, C, 1)).astype(np.float32)).to(dev)
    enc_b = torch.from_numpy(rng.normal(0, 0.5, FEAT).astype(np.float32)).to(dev)
    out = {"metric": "transfusion_proposals_init_decode", "map": [C, H, W], "num_proposals": K, "features": FEAT,
           "device_launches": DEVICE_LAUNCHES, "device_launches_total": sum(DEVICE_LAUNCHES.values())}
    for B in a.batches:
        t = lambda x: torch.from_numpy(x.astype(np.float32)).to(dev)
        logits = t(rng.normal(-4, 2, (B, C, H, W)))
        feat = t(rng.normal(0, 1, (B, FEAT, H * W)))
        preds = {"heatmap": t(rng.normal(0, 2, (B, C, K))), "center": t(rng.uniform(0, 180, (B, 2, K))),
                 "height": t(rng.uniform(-4, 2, (B, 1, K))), "dim": t(rng.normal(0.5, 0.5, (B, 3, K))),
                 "rot": t(rng.normal(0, 1, (B, 2, K))), "vel": t(rng.normal(0, 3, (B, 2, K)))}

        def device_path():
            top_class, top_index, _, qhs = head(logits)
            qf, qp = head.init_queries(feat, pos, enc_w, enc_b, top_class, top_index)
            return dec.get_bboxes({**preds, "query_heatmap_score": qhs}, top_class), qf, qp

        def plain_path():
            top_class, top_index, _, qhs = proposals_plain(logits, K, head.point_classes, stable=False)
            qf, qp = init_queries_plain(feat, pos, enc_w, enc_b, top_class, top_index)
            return get_bboxes_plain({**preds, "query_heatmap_score": qhs}, top_class, dec), qf, qp

        with torch.no_grad():
            got, want = device_path(), plain_path()
            top = head(logits)
            ref = proposals_plain(logits, K, head.point_classes, stable=True)
            res = {"selection_equal_to_stable_plain": bool(torch.equal(top[0], ref[0]) and torch.equal(top[1], ref[1])),
                   "kept_device": [int(d["pred_boxes"].shape[0]) for d in got[0]],
                   "kept_plain": [int(d["pred_boxes"].shape[0]) for d in want[0]],
                   "query_feat_equal": bool(torch.equal(got[1], want[1])), "query_pos_equal": bool(torch.equal(got[2], want[2]))}
            preds_d = {**preds, "query_heatmap_score": top[3]}
            med, lo, hi = events(lambda: head(logits), a.reps, a.inner)
            nbytes = 4 * B * C * H * W
            res.update(proposals_us=med, proposals_p10_us=lo, proposals_p90_us=hi, proposals_read_bytes=nbytes,
                       proposals_GBps=round(nbytes / med / 1e3, 1))
            med, lo, hi = events(lambda: head.init_queries(feat, pos, enc_w, enc_b, top[0], top[1]), a.reps, a.inner)
            nbytes = 2 * 4 * B * FEAT * K + 16 * B * K + 16 * B * K
            res.update(init_queries_us=med, init_queries_p10_us=lo, init_queries_p90_us=hi, init_queries_bytes=nbytes)
            med, lo, hi = events(lambda: dec.decode_padded(preds_d, top[0]), a.reps, a.inner)
            nbytes = 4 * B * K * (12 + 2 + 11)
            res.update(decode_us=med, decode_p10_us=lo, decode_p90_us=hi, decode_bytes=nbytes)
            for _ in range(3):
                device_path(), plain_path()
            td, tp = [], []
            for _ in range(a.reps):                                  # alternate the two paths window by window
                td.append(wall(device_path, a.inner))
                tp.append(wall(plain_path, max(1, a.inner // 5)))
            res.update(end_to_end_device_us=round(float(np.median(td)), 1), end_to_end_plain_us=round(float(np.median(tp)), 1),
                       end_to_end_device_p10_p90_us=[round(float(np.percentile(td, 10)), 1), round(float(np.percentile(td, 90)), 1)],
                       end_to_end_plain_p10_p90_us=[round(float(np.percentile(tp, 10)), 1), round(float(np.percentile(tp, 90)), 1)],
                       plain_over_device=round(float(np.median(tp) / np.median(td)), 2))
            # the proposals alone against the plain proposals alone (the sort), both closed by a synchronisation
            ta, tb = [], []
            for _ in range(a.reps):
                ta.append(wall(lambda: head(logits), a.inner))
                tb.append(wall(lambda: proposals_plain(logits, K, head.point_classes, stable=False), a.inner))
            res.update(proposals_wall_us=round(float(np.median(ta)), 1), proposals_plain_wall_us=round(float(np.median(tb)), 1))
        out[f"b{B}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
