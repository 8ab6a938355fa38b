#!/usr/bin/env python3
"""TransFusion head, decoder layer + prediction heads: the device path (dense_heads.transfusion_decoder.DecoderHead, seven
launches of csrc/tfdecoder.hip) against the plain span (TransformerDecoderLayer.forward_plain + the six heads called plainly,
the reference's torch ops) on the same card, in the same process, alternating.  One JSON line.

workload  N = 180 x 180 = 32 400 BEV cells, K = 200 queries, d_model 128, 8 heads, FFN 256, the six nuScenes heads
          (center 2, height 1, dim 3, rot 2, vel 2, heatmap 10), seeded weights (tests/ref_decoder.py's scales), B = 1 and B = 4.
timing    HIP events around `--inner` back-to-back repetitions, median (p10, p90) over `--reps` groups after warm-up; the two
          paths alternate group by group.  In eval the key position embedding is cached by the device path; the plain path
          recomputes it on every forward, as the reference does.
kernels   each on its own, same events, one stage of fnp_tf_decoder_stages at a time on the workspace of a complete call, raw
          ctypes calls on preallocated buffers: front, self-attention, mid, kv_proj (reads the feature map and the position
          embedding, writes K and V; 2 x 2 x N x 128 x 128 FLOP per scene), the cross attention with its merge (reads K and V
          once: the four waves of a workgroup share them through the cache; 4 x K x N x 128 FLOP per scene), tail; with the
          bytes and FLOP each must move and its shares of 8 TB/s and of 157.3 TFLOP/s; the whole call the same way.
launches  device: read from the code (front, self-attention, mid, kv_proj, cross-attention, merge, tail); plain: counted with
          torch.profiler's kernel events over one forward.

    python tools/bench_decoder.py [--reps 20] [--inner 10] [--batches 1 4]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_decoder as RD  # noqa: E402  (the seeded weight generators)
from findnpropagate_amd import lib  # noqa: E402
from findnpropagate_amd.dense_heads import transfusion_decoder as TD  # noqa: E402
from findnpropagate_amd.model_utils.transfusion_utils import PositionEmbeddingLearned, TransformerDecoderLayer  # noqa: E402

H, W, K, FFN = 180, 180, 200, 256
N = H * W
HBM_BPS, F32_MATRIX_FLOPS = 8.0e12, 157.3e12
DEVICE_LAUNCHES = ["front", "self_attention", "mid", "kv_proj", "cross_attention", "merge", "tail"]


def timed_group(fn, inner):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    z.record()
    z.synchronize()
    return a.elapsed_time(z) * 1e3 / inner


def stats(ts):
    ts = np.sort(ts)
    return round(float(np.median(ts)), 1), round(float(ts[len(ts) // 10]), 1), round(float(ts[-1 - len(ts) // 10]), 1)


def events(fn, reps, inner, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return stats([timed_group(fn, inner) for _ in range(reps)])


def count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as e:          # no tracer in this build of torch: the count is left out, the timings stand
        return f"not counted: {type(e).__name__}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 4])
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = lib.load()
    rng = np.random.default_rng(0)
    dec = TransformerDecoderLayer(RD.D, RD.NHEAD, FFN, 0.1, "relu", self_posembed=PositionEmbeddingLearned(2, RD.D),
                                  cross_posembed=PositionEmbeddingLearned(2, RD.D))
    heads = TD.SeparateHead_Transfusion(RD.D, 64, 1, RD.sep_head_dict(RD.NUSC_HEADS))
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in RD.decoder_weights(0, FFN).items()})
    heads.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in RD.head_weights(0, RD.NUSC_HEADS, False).items()})
    dec, heads = dec.eval().to(dev), heads.eval().to(dev)
    head = TD.DecoderHead(dec, heads)
    bev_pos = torch.from_numpy(RD.create_2d_grid(W, H)[..., ::-1].copy()).to(dev)
    split_len, tile_len = TD.attention_geometry(N)
    out = {"metric": "transfusion_decoder_and_heads", "cells": N, "queries": K, "ffn": FFN, "heads": RD.NUSC_HEADS,
           "split_len": split_len, "tile_len": tile_len, "device_launches": DEVICE_LAUNCHES, "device_launches_total": len(DEVICE_LAUNCHES)}
    t = lambda x: torch.from_numpy(x.astype(np.float32)).to(dev)
    for B in a.batches:
        query, key = t(rng.normal(0, 1, (B, RD.D, K))), t(rng.normal(0, 1, (B, RD.D, N)))
        query_pos = bev_pos[0][torch.from_numpy(rng.integers(0, N, (B, K))).to(dev)].contiguous()
        bev_b = bev_pos.repeat(B, 1, 1)
        with torch.no_grad():
            assert head.plain_reasons(query, key, query_pos, bev_pos) == []
            device_path = lambda: head(query, key, query_pos, bev_pos)
            plain_path = lambda: head.call_plain(query, key, query_pos, bev_b)
            got, want = device_path(), plain_path()
            res = {"max_abs_difference": {k: float((got[k] - want[k]).abs().max()) for k in got}}
            for _ in range(3):
                device_path(), plain_path()
            torch.cuda.synchronize()
            td, tp = [], []
            for _ in range(a.reps):                                  # alternate the two paths group by group
                td.append(timed_group(device_path, a.inner))
                tp.append(timed_group(plain_path, max(1, a.inner // 5)))
            (d, dlo, dhi), (p, plo, phi) = stats(td), stats(tp)
            res.update(device_us=d, device_p10_p90_us=[dlo, dhi], plain_us=p, plain_p10_p90_us=[plo, phi],
                       plain_over_device=round(p / d, 2), plain_launches=count_kernels(plain_path))
            # every kernel on its own: one stage of fnp_tf_decoder_stages at a time on the workspace a complete call left, raw
            # ctypes calls on preallocated buffers (no wrapper, no allocation between the events)
            pack = head.pack
            total_out = sum(pack.head_out)
            ws_bytes = L.fnp_tf_decoder_workspace_bytes(B, K, N, FFN, total_out)
            ws = torch.empty(ws_bytes // 4, device=dev)
            out_feat, out_heads = torch.empty((B, RD.D, K), device=dev), torch.empty(B * K * total_out, device=dev)
            args = (lib.ptr(query), lib.ptr(key), lib.ptr(query_pos), lib.ptr(pack.key_pe), 0, lib.ptr(pack.params), pack.params.numel(),
                    B, K, N, FFN, len(pack.head_out), pack.head_out_c, pack.center, lib.ptr(ws), ws_bytes, lib.ptr(out_feat), lib.ptr(out_heads))
            stream = lib.stream()
            stage = lambda mask: lib.check(L.fnp_tf_decoder_stages(*args, mask, stream), "fnp_tf_decoder_stages")
            stage(63)
            whole = events(lambda: stage(63), a.reps, a.inner)
            res["device_without_wrapper_us"] = whole[0]
            pad = sum((n + 15) // 16 * 16 for n in pack.head_out)
            w = RD.D * RD.D
            work = {   # name: (mask, launches, FLOP, bytes it must move: weights once + activations in and out)
                "front": (1, 1, 2 * B * K * (w + 3 * w), 4 * (4 * w + B * K * (RD.D + 2) + 5 * B * K * RD.D)),
                "self_attention": (2, 1, 4 * B * K * K * RD.D, 4 * 4 * B * K * RD.D),
                "mid": (4, 1, 2 * B * K * 2 * w, 4 * (2 * w + 3 * B * K * RD.D + 2 * B * K * RD.D)),
                "kv_proj": (8, 1, 2 * 2 * B * N * w, 4 * RD.D * N * (B + 1 + 2 * B)),
                "cross_attention_and_merge": (16, 2, 4 * B * K * N * RD.D, 4 * RD.D * (2 * B * N + 2 * B * K)),
                "tail": (32, 1, 2 * B * K * (w + 2 * RD.D * FFN + RD.D * 64 * len(pack.head_out) + 64 * pad),
                         4 * (w + 2 * RD.D * FFN + RD.D * 64 * len(pack.head_out) + 64 * pad + 2 * B * K * RD.D + B * K * (RD.D + total_out))),
            }
            parts = 0.0
            for name, (mask, launches, flops, nbytes) in work.items():
                us, lo, hi = events(lambda m=mask: stage(m), a.reps, a.inner)
                parts += us
                res[name] = dict(us=us, p10_p90_us=[lo, hi], launches=launches, bytes=nbytes, flops=flops,
                                 hbm_share=round(nbytes / (us * 1e-6) / HBM_BPS, 4), matrix_share=round(flops / (us * 1e-6) / F32_MATRIX_FLOPS, 4))
            res["cross_attention_and_merge"]["exps"] = B * K * N * RD.NHEAD
            res["sum_of_kernels_us"] = round(parts, 1)
        out[f"b{B}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
