#!/usr/bin/env python3
"""Secondary measurement ((f)1): the hand-off from the sparse backbone to the dense BEV backbone on B synthetic scenes —
the reference's way (SparseConvTensor.dense() -> view -> ZeroPad2d + Conv2d(256 -> 128, 3x3) + BatchNorm2d + ReLU as torch /
MIOpen modules) against the first block evaluated on the sparse rows (fnp_rulebook_strided + fnp_spconv_forward with the
BatchNorm / ReLU epilogue + fnp_sparse_to_dense_fill).  One JSON line.

--train: forward + backward of the same hand-off in train() to a scalar loss on the block's output — the reference way
(differentiable HeightCompression + torch's blocks[0][:4]) against FNP_SPARSE_FIRST_TRAIN's route (rulebook, SparseConvFunction,
bev_bn_act: no dense input map), with f32 rows and under torch.autocast(float16), at 16 single-sweep scenes and at the 4 ten-sweep
scenes of tools/bench_train.py; the two ways alternate in one process, device events around --reps repetitions after a warm-up,
three rounds, medians; torch.cuda.max_memory_allocated of each.  One JSON line."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from findnpropagate_amd import sparse as S, synthetic as syn
from findnpropagate_amd.backbones_2d import BaseBEVBackbone, HeightCompression
from findnpropagate_amd.backbones_3d import VoxelResBackBone8x

ap = argparse.ArgumentParser(); ap.add_argument("--batch", type=int, default=16); ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--train", action="store_true", help="forward + backward in train(): the reference way against FNP_SPARSE_FIRST_TRAIN")
ap.add_argument("--shapes", default="16x1,4x10", help="--train: scenes x sweeps of each shape (a kernel trace of one shape: --shapes 16x1)")
args = ap.parse_args()
dev = torch.device("cuda", 0); B = args.batch
grid = np.round((np.array(syn.POINT_CLOUD_RANGE[3:]) - np.array(syn.POINT_CLOUD_RANGE[:3])) / np.array(syn.VOXEL_SIZE)).astype(int)
net3d = syn.init_backbone_weights(VoxelResBackBone8x({"USE_BIAS": False}, 5, grid), 0).to(dev).eval()
bev = BaseBEVBackbone({"LAYER_NUMS": [5, 5], "LAYER_STRIDES": [1, 2], "NUM_FILTERS": [128, 256], "UPSAMPLE_STRIDES": [1, 2],
                       "NUM_UPSAMPLE_FILTERS": [256, 256], "USE_CONV_FOR_NO_STRIDE": True}, 256).to(dev).eval()
hc = HeightCompression({"NUM_BEV_FEATURES": 256, "REUSE_OUTPUT": True})
BEV_CFG = {"LAYER_NUMS": [5, 5], "LAYER_STRIDES": [1, 2], "NUM_FILTERS": [128, 256], "UPSAMPLE_STRIDES": [1, 2],
           "NUM_UPSAMPLE_FILTERS": [256, 256], "USE_CONV_FOR_NO_STRIDE": True}


def train_mode():
    reps = max(args.reps, 20)
    hc_t = HeightCompression({"NUM_BEV_FEATURES": 256})
    ref = BaseBEVBackbone(dict(BEV_CFG), 256).to(dev).train()
    new = BaseBEVBackbone(dict(BEV_CFG, FNP_SPARSE_FIRST_TRAIN=True), 256).to(dev).train()
    new.load_state_dict(ref.state_dict())
    shapes = []
    for scenes, sweeps in (tuple(int(v) for v in sh.split("x")) for sh in args.shapes.split(",")):
        pts, off = syn.make_sweeps_batch(list(range(scenes)), sweeps) if sweeps > 1 else syn.make_batch(list(range(scenes)))
        cfg = S.make_voxel_cfg(syn.VOXEL_SIZE, syn.POINT_CLOUD_RANGE, 5, 10, 120000 if sweeps > 1 else 160000)
        with torch.no_grad():
            t = net3d.forward_points(torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev), scenes, cfg)["out"]
        feats = t.features.float().detach().clone().requires_grad_(True)          # the reference boundary: f32 rows
        t = t.replace_feature(feats)
        t.rank_grid(), t.n_dev()
        entry = {"scenes": scenes, "sweeps": sweeps, "encoded_rows": int(feats.shape[0])}
        for label, amp in (("f32_rows", False), ("autocast_fp16", True)):
            def way(net, sparse):
                for p in (feats, net.blocks[0][1].weight, net.blocks[0][2].weight, net.blocks[0][2].bias):
                    p.grad = None
                with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
                    if sparse:
                        assert not net.sparse_train_reasons({"encoded_spconv_tensor": t})
                        y = net.first_block_train(t)
                    else:
                        y = net.blocks[0][:4](hc_t({"encoded_spconv_tensor": t, "encoded_spconv_tensor_stride": 8})["spatial_features"])
                    loss = (y.float() ** 2).mean()
                loss.backward()
                return y
            ways = {"reference_way": lambda: way(ref, False), "from_sparse_rows": lambda: way(new, True)}
            ms, peak = {k: [] for k in ways}, {}
            for rnd in range(3):
                for k, fn in ways.items():
                    for _ in range(3): fn()
                    torch.cuda.synchronize()
                    if rnd == 0: torch.cuda.reset_peak_memory_stats()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps): y = fn()
                    e1.record(); torch.cuda.synchronize()
                    ms[k].append(e0.elapsed_time(e1) / reps)
                    if rnd == 0: peak[k] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
                    del y
            med = {k: float(np.median(v)) for k, v in ms.items()}
            entry[label] = {"reference_way_ms": round(med["reference_way"], 4), "from_sparse_rows_ms": round(med["from_sparse_rows"], 4),
                            "rounds_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                            "speedup": round(med["reference_way"] / med["from_sparse_rows"], 2), "max_memory_allocated_MiB": peak}
        shapes.append(entry)
        del t, feats
    print(json.dumps({"workload": "first BaseBEVBackbone block behind the sparse backbone in train(): forward + backward to a scalar loss on its "
                                  "output ((B,128,2,180,180) rows -> (B,128,180,180))", "reps": reps, "rounds": 3, "shapes": shapes}))


if args.train:
    train_mode()
    sys.exit(0)
pts, off = syn.make_batch(list(range(B)))
cfg = S.make_voxel_cfg(syn.VOXEL_SIZE, syn.POINT_CLOUD_RANGE, 5, 10, 160000)
with torch.no_grad():
    r = net3d.forward_points(torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev), B, cfg)
t = r["out"]
t = t.replace_feature(t.features.float())      # the reference boundary: f32 rows


def timed(fn):
    with torch.no_grad():
        for _ in range(3): fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for _ in range(args.reps): out = fn()
        e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps, out


def dense_way():
    d = hc({"encoded_spconv_tensor": t, "encoded_spconv_tensor_stride": 8})["spatial_features"]
    return bev.blocks[0][:4](d)


ms_dense_only, _ = timed(lambda: hc({"encoded_spconv_tensor": t, "encoded_spconv_tensor_stride": 8})["spatial_features"])
ms_dense, want = timed(dense_way)
ms_sparse, got = timed(lambda: bev.first_block_from_sparse(t))
t16 = t.replace_feature(t.features.bfloat16())
ms_sparse16, got16 = timed(lambda: bev.first_block_from_sparse(t16))
err = float((got - want).abs().max() / want.abs().max().clamp(min=1.0))
print(json.dumps({"workload": "first BaseBEVBackbone block behind the sparse backbone: (B,128,2,180,180) rows -> (B,128,180,180) f32",
                  "scenes": B, "encoded_rows": int(t.features.shape[0]), "reference_way_ms": {"dense_map_write": round(ms_dense_only, 4), "dense_map + torch conv/bn/relu (f32)": round(ms_dense, 4)},
                  "from_sparse_rows_ms": {"f32_rows": round(ms_sparse, 4), "bf16_rows": round(ms_sparse16, 4)},
                  "speedup_f32": round(ms_dense / ms_sparse, 2), "max_rel_err_f32_vs_torch": err}))
