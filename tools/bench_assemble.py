#!/usr/bin/env python3
"""Multi-sweep assembly on the device against the host and against prepare_points: one JSON line.

device: sparse.assemble_sweeps (fnp_assemble_sweeps) on synthetic.make_raw_sweeps samples (10 sweeps, ~330 k raw rows each),
        median of HIP-event timed launches after warm-up, for B = 128 scenes (--distinct seeded samples, cycled) and B = 1; in the
        same process sparse.prepare_points on the same row count and scene count (fnp_prepare_points, the kernels with the same
        pass structure): without a program and without shuffle, and with the four-op program and the device shuffle.
        rate: the algorithmic bytes, R x 28 B read (x, y in the mark, the row in the emit) + kept x 20 B written, over the time;
        and the bytes the kernels request, R x 40 B (the mark stages whole rows too) + kept x 20 B (moved_bytes).
host:   datasets.nuscenes_sweeps.assemble_host (the reference's numpy arithmetic) per scene, median, in a child process held to
        one thread — what a DataLoader worker of the reference pays per sample.  Runs first, before this process touches the GPU.

    python tools/bench_assemble.py [--reps 50] [--scenes 128] [--distinct 16]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from findnpropagate_amd import synthetic as syn  # noqa: E402
from findnpropagate_amd.datasets import nuscenes_sweeps as NS  # noqa: E402

CFG = [dict(NAME='random_world_flip', ALONG_AXIS_LIST=['x', 'y']),
       dict(NAME='random_world_rotation', WORLD_ROT_ANGLE=[-0.78539816, 0.78539816]),
       dict(NAME='random_world_scaling', WORLD_SCALE_RANGE=[0.9, 1.1]),
       dict(NAME='random_world_translation', NOISE_TRANSLATE_STD=[0.5, 0.5, 0.5])]


def host_only(distinct, reps):
    scenes = [syn.make_raw_sweeps(s) for s in range(min(distinct, 4))]
    ts = []
    for _ in range(reps):
        for sc in scenes:
            t = time.perf_counter()
            NS.assemble_host(sc)
            ts.append(time.perf_counter() - t)
    print(json.dumps({"host_ms_per_scene": round(float(np.median(ts)) * 1e3, 2),
                      "host_raw_rows_per_scene": int(np.mean([sum(s[0].shape[0] for s in sc) for sc in scenes]))}))


def timed(fn, reps, warmup=10):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        z.record()
        z.synchronize()
        ts.append(a.elapsed_time(z) * 1e3)
    ts = np.sort(ts)
    return float(np.median(ts)), float(ts[len(ts) // 10]), float(ts[-1 - len(ts) // 10])


def device(scenes, reps):
    import torch

    from findnpropagate_amd import sparse as S
    from findnpropagate_amd.augmentor.data_augmentor import DataAugmentor, PROGRAM_KEY, stack_programs

    dev = torch.device("cuda", 0)
    B = len(scenes)
    packed = NS.pack_sweeps(scenes)
    args = [torch.from_numpy(a).to(dev) for a in packed]
    R = int(packed[0].shape[0])
    out = S.assemble_sweeps(*args, B)
    kept = int(out["n"].item())
    res = {"scenes": B, "sweeps": int(packed[4].shape[0]), "raw_rows": R, "kept": kept}
    med, lo, hi = timed(lambda: S.assemble_sweeps(*args, B, out=out), reps)
    nbytes, moved = R * 28 + kept * 20, R * 40 + kept * 20
    res.update(assemble_us=round(med, 1), assemble_p10_us=round(lo, 1), assemble_p90_us=round(hi, 1),
               algorithmic_bytes=nbytes, assemble_GBps=round(nbytes / med / 1e3, 1),
               moved_bytes=moved, assemble_moved_GBps=round(moved / med / 1e3, 1))
    # prepare_points on the same rows: the raw rows as points, the scenes' raw row ranges as offsets
    off = torch.from_numpy(packed[1][packed[2]].astype(np.int32)).to(dev)
    progs = []
    for b in range(B):
        np.random.seed(b)
        progs.append(DataAugmentor(None, CFG, [], deferred=True).forward(dict(points=np.zeros((1, 5), np.float32),
                                                                              gt_boxes=np.zeros((0, 9), np.float32)))[PROGRAM_KEY])
    prog = torch.from_numpy(stack_programs(progs)).to(dev)
    for name, p, shuffle in (("prepare_plain", None, None), ("prepare_program_shuffle", prog, "device")):
        o = S.prepare_points(args[0], off, B, p, syn.POINT_CLOUD_RANGE, shuffle=shuffle)
        med, lo, hi = timed(lambda: S.prepare_points(args[0], off, B, p, syn.POINT_CLOUD_RANGE, shuffle=shuffle, out=o), reps)
        res.update({name + "_us": round(med, 1), name + "_p10_us": round(lo, 1), name + "_p90_us": round(hi, 1),
                    name + "_kept": int(o["n"].item())})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--scenes", type=int, default=128)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    if a.host_only:
        host_only(a.distinct, 5)
        return
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    host = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-only", "--distinct", str(a.distinct)], env=env,
                          capture_output=True, text=True, check=True).stdout.strip().splitlines()[-1]
    out = {"metric": "assemble_sweeps", **json.loads(host)}
    distinct = [syn.make_raw_sweeps(s) for s in range(min(a.distinct, a.scenes))]
    out[f"b{a.scenes}"] = device([distinct[b % len(distinct)] for b in range(a.scenes)], a.reps)
    out["b1"] = device(distinct[:1], a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
