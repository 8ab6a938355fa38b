#!/usr/bin/env python3
"""The differentiable attention core, forward + backward: dense_heads.transfusion_decoder.attention_autograd
(fnp_tf_attention_stats, then csrc/tfattn_grad.hip) against the same span as torch ops (softmax(0.25 q k^T) v per head with
torch's autograd: the core of nn.MultiheadAttention without its projections) on the same card, in the same process,
alternating.  One JSON line.

workload  K = 200 queries over N = 180 x 180 = 32 400 keys, 8 heads of 16, N(0, 1) inputs, B = 1 and B = 4; q, k and v all
          require a gradient.
timing    HIP events around `--inner` back-to-back repetitions, median (p10, p90) over `--reps` groups after warm-up; the two
          paths alternate group by group.  A repetition is forward + backward through autograd, allocations included.
kernels   the library's calls on their own, same events, raw ctypes calls on preallocated buffers: the forward with statistics
          (attention kernel + merge), the backward asked for dq alone (D prologue, query-stationary kernel, merge), for dk and
          dv alone (D prologue, key-stationary kernel), and for all three; with the FLOP each performs (2 x K x N x 16 per
          head and product: 2 products forward, 3 for dq, 4 for dk and dv) and its share of 157.3 TFLOP/s.
memory    torch.cuda.max_memory_allocated over one forward + backward of either path, above what was allocated before it
          (inputs, d_out); one score tensor is 8 x K x N x 4 bytes per scene.
dropout   --dropout P (0 < P < 1): the fused span is attention_autograd(q, k, v, P, seed) (the dropout instantiations of the three
          kernels, the mask regenerated from one seed on the device), the torch span the same expression with F.dropout(P) on the
          probabilities, and the kernels on their own are the fnp_tf_attention_dropout_* calls.  The two spans draw different
          masks, so no difference of gradients is reported (tests/test_gpu_attention_dropout.py holds the values).  Without
          --dropout every call is the plain one: run both in one session to see what the mask costs per kernel.

    python tools/bench_attention_grad.py [--reps 20] [--inner 5] [--batches 1 4] [--dropout 0.1]
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

import ref_attention_grad as RG  # noqa: E402  (the torch expression)
from findnpropagate_amd import lib  # noqa: E402
from findnpropagate_amd.dense_heads import transfusion_decoder as TD  # noqa: E402

K, N, D, HEADS = 200, 180 * 180, 128, 8
F32_MATRIX_FLOPS = 157.3e12


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


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 4])
    ap.add_argument("--dropout", type=float, default=0.0)
    a = ap.parse_args()
    P = a.dropout
    assert 0.0 <= P < 1.0
    dev = torch.device("cuda", 0)
    L = lib.load()
    rng = np.random.default_rng(0)
    out = {"metric": "attention_core_forward_backward", "queries": K, "keys": N, "split_len": TD.attention_geometry(N)[0],
           "backward_key_block": TD.attention_backward_geometry(N)[0], "dropout_p": P}
    seed = torch.tensor([0x0123456789ABCDEF], dtype=torch.int64, device=dev)

    def torch_dropout(q, k, v):
        B = q.shape[0]
        heads = lambda t, rows: t.reshape(B, rows, HEADS, 16).transpose(1, 2)
        p = torch.softmax(0.25 * (heads(q, K) @ heads(k, N).transpose(2, 3)), dim=-1)
        return (torch.nn.functional.dropout(p, P) @ heads(v, N)).transpose(1, 2).reshape(B, K, D)

    t = lambda *shape: torch.from_numpy(rng.normal(0, 1, shape).astype(np.float32)).to(dev)
    for B in a.batches:
        q, k, v, d_out = t(B, K, D), t(B, N, D), t(B, N, D), t(B, K, D)
        q.requires_grad_(), k.requires_grad_(), v.requires_grad_()

        def span(fn):
            q.grad = k.grad = v.grad = None
            fn(q, k, v).backward(d_out)

        if P > 0:
            fused, plain = (lambda: span(lambda *x: TD.attention_autograd(*x, P, seed))), (lambda: span(torch_dropout))
            res = {}
        else:
            fused, plain = (lambda: span(TD.attention_autograd)), (lambda: span(RG.attention_torch))
            fused()
            got = [x.grad.clone() for x in (q, k, v)]
            plain()
            res = {"max_abs_difference": {n: float((g - x.grad).abs().max()) for n, g, x in zip(("dq", "dk", "dv"), got, (q, k, v))}}
            q.grad = k.grad = v.grad = None
            del got
        res["score_tensor_bytes"] = HEADS * K * N * 4 * B
        res["fused_peak_bytes"], res["torch_peak_bytes"] = peak(fused), peak(plain)
        for _ in range(3):
            fused(), plain()
        torch.cuda.synchronize()
        tf, tp = [], []
        for _ in range(a.reps):                                      # alternate the two paths group by group
            tf.append(timed_group(fused, a.inner))
            tp.append(timed_group(plain, a.inner))
        (f, flo, fhi), (p, plo, phi) = stats(tf), stats(tp)
        res.update(fused_us=f, fused_p10_p90_us=[flo, fhi], torch_us=p, torch_p10_p90_us=[plo, phi], torch_over_fused=round(p / f, 2))
        # the library's calls on their own: preallocated buffers, no wrapper, no allocation between the events
        with torch.no_grad():
            qd, kd, vd = q.detach(), k.detach(), v.detach()
            o, st = TD.attention_stats(qd, kd, vd, dropout_p=P, seed=seed)
            dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
            fw_bytes, bw_bytes = L.fnp_tf_attention_workspace_bytes(B, K, N), L.fnp_tf_attention_backward_workspace_bytes(B, K, N)
            fw, bw = torch.empty(fw_bytes // 4, device=dev), torch.empty(bw_bytes // 4, device=dev)
            stream = lib.stream()
            forward = lambda: lib.check(L.fnp_tf_attention_stats(lib.ptr(qd), lib.ptr(kd), lib.ptr(vd), B, K, N, lib.ptr(fw), fw_bytes,
                                                                 lib.ptr(o), lib.ptr(st), stream), "fnp_tf_attention_stats")
            backward = lambda a_, b_, c_: lib.check(L.fnp_tf_attention_backward(
                lib.ptr(qd), lib.ptr(kd), lib.ptr(vd), lib.ptr(o), lib.ptr(st), lib.ptr(d_out), B, K, N, lib.ptr(bw), bw_bytes,
                lib.ptr(a_), lib.ptr(b_), lib.ptr(c_), stream), "fnp_tf_attention_backward")
            if P > 0:
                forward = lambda: lib.check(L.fnp_tf_attention_dropout_stats(
                    lib.ptr(qd), lib.ptr(kd), lib.ptr(vd), B, K, N, lib.ptr(fw), fw_bytes, lib.ptr(o), lib.ptr(st), P, lib.ptr(seed),
                    stream), "fnp_tf_attention_dropout_stats")
                backward = lambda a_, b_, c_: lib.check(L.fnp_tf_attention_dropout_backward(
                    lib.ptr(qd), lib.ptr(kd), lib.ptr(vd), lib.ptr(o), lib.ptr(st), lib.ptr(d_out), B, K, N, lib.ptr(bw), bw_bytes,
                    lib.ptr(a_), lib.ptr(b_), lib.ptr(c_), P, lib.ptr(seed), stream), "fnp_tf_attention_dropout_backward")
            product = 2 * B * K * N * D
            calls = {"forward_with_stats": (forward, 2), "backward_dq": (lambda: backward(dq, None, None), 3),
                     "backward_dk_dv": (lambda: backward(None, dk, dv), 4), "backward_all": (lambda: backward(dq, dk, dv), 7)}
            for name, (fn, products) in calls.items():
                us, lo, hi = events(fn, a.reps, a.inner)
                res[name] = dict(us=us, p10_p90_us=[lo, hi], flops=products * product,
                                 matrix_share=round(products * product / (us * 1e-6) / F32_MATRIX_FLOPS, 4))
            res["workspace_bytes"] = {"forward": fw_bytes, "backward": bw_bytes}
        out[f"b{B}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
