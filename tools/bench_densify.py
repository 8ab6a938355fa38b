#!/usr/bin/env python3
"""Time the dense map of HeightCompression forward (fnp_sparse_to_dense) and backward (fnp_sparse_to_dense_backward) on the
backbone's real encoded tensor, against the torch adjoint the reference's spconv runs (autograd of its index assignment:
index_put backward = a gather from the channels-first gradient).  HIP events, median of per-call times.  Shapes:
  train: 4 synthetic 10-sweep scenes, fp16 rows (the shipped training step under AMP);
  eval16: 16 one-sweep scenes, f32 and bf16 rows.
Bytes: `map` = the whole dense tensor; `tile` = the gradient-map bytes of the 64*VEC-cell tiles that hold a row (what the
backward reads at most) + the row bytes it writes.  Development tool."""
import argparse, os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from findnpropagate_amd import sparse as S, synthetic as syn, lib as _l
from findnpropagate_amd.backbones_3d import VoxelResBackBone8x

ap = argparse.ArgumentParser(); ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--shapes", default="train,eval16")
args = ap.parse_args()
dev = torch.device("cuda", 0)
grid = np.round((np.array(syn.POINT_CLOUD_RANGE[3:]) - np.array(syn.POINT_CLOUD_RANGE[:3])) / np.array(syn.VOXEL_SIZE)).astype(int)
L = _l.load()


def encoded(B, sweeps):
    net = syn.init_backbone_weights(VoxelResBackBone8x({"USE_BIAS": False}, 5, grid), 0).to(dev).eval()
    pts, off = syn.make_sweeps_batch(list(range(B)), sweeps) if sweeps > 1 else syn.make_batch(list(range(B)))
    cfg = S.make_voxel_cfg(syn.VOXEL_SIZE, syn.POINT_CLOUD_RANGE, 5, 10, 120000 if sweeps > 1 else 160000)
    with torch.no_grad():
        t = net.forward_points(torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev), B, cfg)["out"]
    return t


def timed(fn):
    for _ in range(3): fn()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
    torch.cuda.synchronize(); evs[0].record()
    for i in range(args.reps):
        fn(); evs[i + 1].record()
    torch.cuda.synchronize()
    return float(np.median([evs[i].elapsed_time(evs[i + 1]) for i in range(args.reps)]))


def run(name, t, dtype):
    f = t.features.detach().to(dtype).contiguous()
    idx, n_dev, B, shape = t.indices, t.n_dev(), t.batch_size, list(t.spatial_shape)
    n, C, es = int(n_dev.item()), f.shape[1], f.element_size()
    ws = torch.empty((int(L.fnp_sparse_to_dense_workspace_bytes(B, *shape)),), dtype=torch.uint8, device=dev)
    out = torch.empty((B, C, *shape), dtype=dtype, device=dev)
    G = torch.randn((B, C, *shape), device=dev).to(dtype)
    fwd = lambda: S.to_dense(f, idx, n_dev, B, shape, workspace=ws, out=out)
    bwd = lambda: S.dense_backward(G, idx, n_dev, B, shape, workspace=ws)
    # the reference's dense(): zeros + index assignment, channels-last permuted to channels-first; its backward is torch's
    fr = f[:n].clone().requires_grad_(True)
    i = idx[:n].long()
    ref = torch.zeros((B, *shape, C), dtype=dtype, device=dev).index_put((i[:, 0], i[:, 1], i[:, 2], i[:, 3]), fr).permute(0, 4, 1, 2, 3)
    assert torch.equal(bwd()[:n], torch.autograd.grad(ref, fr, G, retain_graph=True)[0]), "adjoint differs from torch's"
    ms_f, ms_b = timed(fwd), timed(bwd)
    ms_t = timed(lambda: torch.autograd.grad(ref, fr, G, retain_graph=True))
    # tiles (64 * VEC cells of a (b, z) plane, VEC 2 on these planes) that hold at least one row
    ci = idx[:n].cpu().numpy().astype(np.int64)
    plane = shape[1] * shape[2]
    tiles = np.unique((ci[:, 0] * shape[0] + ci[:, 1]) * ((plane + 127) // 128) + (ci[:, 2] * shape[2] + ci[:, 3]) // 128).shape[0]
    map_b = B * C * shape[0] * plane * es
    tile_b = tiles * 128 * C * es + n * C * es
    return {"shape": name, "dtype": str(dtype).replace("torch.", ""), "batch": B, "rows": n, "C": C, "grid": shape, "map_MB": round(map_b / 1e6, 1),
            "occupied_tiles": tiles, "tiles": B * shape[0] * ((plane + 127) // 128), "bwd_bytes_MB": round(tile_b / 1e6, 1),
            "fwd_ms": round(ms_f, 4), "fwd_GBs": round(map_b / ms_f / 1e6, 1), "bwd_ms": round(ms_b, 4), "bwd_GBs": round(tile_b / ms_b / 1e6, 1),
            "bwd_over_fwd": round(ms_b / ms_f, 3), "torch_adjoint_ms": round(ms_t, 4), "torch_over_bwd": round(ms_t / ms_b, 2)}


res = []
if "train" in args.shapes:
    res.append(run("train_4x10sweep_amp", encoded(4, 10), torch.float16))
if "eval16" in args.shapes:
    t = encoded(16, 1)
    for dt in (torch.float32, torch.bfloat16):
        res.append(run("16x1sweep", t, dt))
for r in res:
    print(json.dumps(r))
