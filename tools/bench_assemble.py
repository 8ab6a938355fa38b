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

raw-scene augmentor (key "raw_scenes", same process, after the above):
        window  sparse.assemble_sweeps(window=) (fnp_assemble_sweeps_window) on the B scenes with 2 000 finished lead rows each,
                INTERLEAVED launch by launch with the plain entry on the same scenes without them;
        rows    sparse.rows_in_boxes at 4 ten-sweep scenes x 40 boxes (and the host form on the same scenes, one thread);
        chain   the input chain of 4 scenes from raw sweeps to prepared points, wall clock with a device synchronisation at the
                end, interleaved: the device route (upload raw, assemble with windows, rows_in_boxes + copy per scene, assemble
                again with 1 500 tail rows, prepare_points with the cut 4-tuple) against the route without it (numpy assembly,
                the host rows-in-boxes per scene, lead | scene | tail joined in numpy, upload, prepare_points with the same cut).
                The augmentor's own Python (sampling policy, queue, box arithmetic) is the same in both routes and in neither.

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


def interleaved(fns, reps, warmup=10):
    """HIP-event medians (us) of several launch sequences timed in turn, launch by launch"""
    import torch

    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            z.record()
            z.synchronize()
            ts[k].append(a.elapsed_time(z) * 1e3)
    return [(round(float(np.median(t)), 1), round(float(np.sort(t)[len(t) // 10]), 1), round(float(np.sort(t)[-1 - len(t) // 10]), 1))
            for t in ts]


def wall(fns, reps, warmup=3):
    """wall-clock medians (ms) of several host + device routes run in turn, each closed by a device synchronisation"""
    import torch

    ts = [[] for _ in fns]
    for r in range(warmup + reps):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warmup:
                ts[k].append((time.perf_counter() - t) * 1e3)
    return [round(float(np.median(t)), 3) for t in ts]


def boxes_on(rng, n, scene_rows):
    b = np.zeros((n, 7), np.float32)
    b[:, 0:3] = scene_rows[rng.integers(0, scene_rows.shape[0], n), 0:3]
    b[:, 3:6] = rng.uniform([1.5, 0.6, 1.0], [5.0, 2.2, 2.5], (n, 3))
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b


def raw_scenes(scenes, four, reps):
    import torch

    from findnpropagate_amd import sparse as S
    from findnpropagate_amd.augmentor import database_sampler as DS
    from findnpropagate_amd.augmentor.data_augmentor import stack_cut_boxes
    from findnpropagate_amd.augmentor.pseudo_loader import points_in_boxes_compact

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    up = lambda arrays: [torch.from_numpy(a).to(dev) for a in arrays]
    rows_at = lambda bx, n: np.concatenate([bx[rng.integers(0, bx.shape[0], n), :3], rng.uniform(0, 1, (n, 2))], 1).astype(np.float32)
    res = {}
    # window entry with lead rows | plain entry, same scenes
    B = len(scenes)
    lead = [rng.uniform(-40, 40, (2000, 5)).astype(np.float32) for _ in range(B)]
    plain, win = up(NS.pack_sweeps(scenes)), up(NS.pack_sweeps(scenes, lead=lead))
    o_plain, o_win = S.assemble_sweeps(*plain, B), S.assemble_sweeps(*win[:6], B, window=win[6])
    (a, b) = interleaved([lambda: S.assemble_sweeps(*plain, B, out=o_plain),
                          lambda: S.assemble_sweeps(*win[:6], B, window=win[6], out=o_win)], reps)
    res["window"] = {"scenes": B, "lead_rows_per_scene": 2000, "plain_us": a[0], "plain_p10_us": a[1], "plain_p90_us": a[2],
                     "window_us": b[0], "window_p10_us": b[1], "window_p90_us": b[2]}
    # rows_in_boxes at 4 scenes x 40 boxes
    host_scenes = [NS.assemble_host(sc) for sc in four]
    copy_boxes = [boxes_on(rng, 40, h) for h in host_scenes]
    cut_boxes = [boxes_on(rng, 39, h) for h in host_scenes]
    lead4 = [rows_at(cb, 2000) for cb in cut_boxes]
    tail4 = [rows_at(cb, 1500) for cb in cut_boxes]
    w4 = up(NS.pack_sweeps(four, lead=lead4))
    a4 = S.assemble_sweeps(*w4[:6], 4, window=w4[6])
    rec, box_off = up(stack_cut_boxes(copy_boxes, [0] * 4)[:2])
    cut = tuple(up(stack_cut_boxes(cut_boxes, [0] * 4)[:2])) + (a4["cut_from"], a4["cut_to"])
    o_rows = S.rows_in_boxes(a4["points"], a4["batch_offsets"], 4, rec, box_off, cut=cut, capacity=1 << 16)
    (r,) = interleaved([lambda: S.rows_in_boxes(a4["points"], a4["batch_offsets"], 4, rec, box_off, cut=cut, capacity=1 << 16, out=o_rows)], reps)
    t = time.perf_counter()
    for h, l, cb, kb in zip(host_scenes, lead4, copy_boxes, cut_boxes):
        points_in_boxes_compact(np.concatenate([l, h]), cb, cut=(DS.cut_records(kb), l.shape[0], l.shape[0] + h.shape[0]))
    res["rows"] = {"scenes": 4, "boxes_per_scene": 40, "rows": int(a4["n"].item()), "inside": int(o_rows["total"].item()),
                   "rows_in_boxes_us": r[0], "rows_in_boxes_p10_us": r[1], "rows_in_boxes_p90_us": r[2],
                   "host_ms_4_scenes": round((time.perf_counter() - t) * 1e3, 2)}
    # the input chain of 4 scenes
    pcr = syn.POINT_CLOUD_RANGE
    cut_np = stack_cut_boxes(cut_boxes, [0] * 4)[:2]

    def device_route():
        w = up(NS.pack_sweeps(four, lead=lead4))
        a = S.assemble_sweeps(*w[:6], 4, window=w[6])
        for b in range(4):
            NS.DeviceSceneRows(a, b, capacity=1 << 14)(copy_boxes[b], cut_boxes[b])
        w = up(NS.pack_sweeps(four, lead=lead4, tail=tail4))
        a = S.assemble_sweeps(*w[:6], 4, window=w[6])
        return S.prepare_points(a["points"], a["batch_offsets"], 4, None, pcr, shuffle="device",
                                cut=tuple(up(cut_np)) + (a["cut_from"], a["cut_to"]))

    def host_route():
        joined, lo, hi = [], [], []
        for sc, l, t_, cb, kb in zip(four, lead4, tail4, copy_boxes, cut_boxes):
            h = NS.assemble_host(sc)
            pts = np.concatenate([l, h])
            points_in_boxes_compact(pts, cb, cut=(DS.cut_records(kb), l.shape[0], pts.shape[0]))
            joined.append(np.concatenate([pts, t_]))
            lo.append(l.shape[0])
            hi.append(pts.shape[0])
        off = np.concatenate([[0], np.cumsum([j.shape[0] for j in joined])]).astype(np.int32)
        p, o = up([np.concatenate(joined), off])
        return S.prepare_points(p, o, 4, None, pcr, shuffle="device", cut=tuple(up(cut_np + (np.array(lo, np.int32), np.array(hi, np.int32)))))

    assert int(device_route()["n"].item()) == int(host_route()["n"].item())
    d, h = wall([device_route, host_route], max(5, reps // 5))
    res["chain"] = {"scenes": 4, "device_route_ms": d, "host_route_ms": h}
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
    out["raw_scenes"] = raw_scenes([distinct[b % len(distinct)] for b in range(a.scenes)], distinct[:4], a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
