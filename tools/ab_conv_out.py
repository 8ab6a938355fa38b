#!/usr/bin/env python3
"""Development (GPU box): same-process, interleaved A/B of conv_out's launch (fnp_spconv_forward, 128 -> 128, K = 3, no residual)
across several builds of the library, on the real conv_out rulebook of a B-scene forward.

The rulebook is made once with the shipped library; every variant (tools/build_head_lib.sh: libfnp_abhead.so, the parent commit's
generic table kernel; tools/build_variant.sh: libfnp_<name>.so) is loaded with ctypes and launched on the SAME device buffers in
interleaved rounds, its output compared bit for bit with the shipped library's.  --caps times the launch on a prefix of the table
(rows and capacity both cut to each value): with a variant built with -DFNP_OUT128_MIN_CAP=1 that is the new kernel below the shipped
dispatch threshold, which is how the threshold was chosen.
usage: tools/ab_conv_out.py --batch 128 --variants abhead[,o1] [--caps 16384,32768,65536] [--out f32|16]"""
import argparse, ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from findnpropagate_amd import lib as _l, sparse as S, synthetic as syn
from findnpropagate_amd.backbones_3d import VoxelResBackBone8x

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128); ap.add_argument("--variants", default="abhead"); ap.add_argument("--caps", default="")
ap.add_argument("--rounds", type=int, default=10); ap.add_argument("--reps", type=int, default=20); ap.add_argument("--warm-rounds", type=int, default=2)
ap.add_argument("--out", default="f32", choices=["f32", "16"], help="output dtype: f32 (what the backbone's last layer writes) or the input's")
args = ap.parse_args()
dev = torch.device("cuda", 0)
B = args.batch
grid = np.round((np.array(syn.POINT_CLOUD_RANGE[3:]) - np.array(syn.POINT_CLOUD_RANGE[:3])) / np.array(syn.VOXEL_SIZE)).astype(int)
net = syn.init_backbone_weights(VoxelResBackBone8x({"USE_BIAS": False}, 5, grid), 0).to(dev).eval()
pts, off = syn.make_batch(list(range(B)))
pts, off = torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)
cfg = S.make_voxel_cfg(syn.VOXEL_SIZE, syn.POINT_CLOUD_RANGE, 5, 10, 160000)
eng = net.engine()
with torch.no_grad():
    net.forward_points(pts, off, B, cfg)
    eng.rulebook_log = []
    net.forward_points(pts, off, B, cfg)
log, eng.rulebook_log = eng.rulebook_log, None
(tag, rb, n_dev), = [e for e in log if e[0][:3] == (128, 128, 3)]
n_full = int(n_dev.item())

libs = {"main": _l.load()}
for v in [v for v in args.variants.split(",") if v]:
    libs[v] = ctypes.CDLL(os.path.join(ROOT, "findnpropagate_amd", "csrc", "ab", f"libfnp_{v}.so"))
for L in libs.values():
    L.fnp_spconv_forward.restype = ctypes.c_int
P, I = ctypes.c_void_p, ctypes.c_int
n_in = int(rb.nbr[:, :n_full].max().item()) + 1
x = torch.randn((n_in, 128), device=dev).to(torch.bfloat16)
w = (torch.randn((3, 128, 128), device=dev) * 0.05).to(torch.bfloat16)
sc, sh = torch.rand(128, device=dev) + 0.5, torch.randn(128, device=dev) * 0.1
odt = torch.float32 if args.out == "f32" else torch.bfloat16
stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

for cap in [int(c) for c in args.caps.split(",") if c] + [rb.cap_out]:
    n = min(n_full, cap)
    nd = S.device_scalar(n, dev)
    outs = {k: torch.zeros((cap, 128), dtype=odt, device=dev) for k in libs}

    def launch(name):
        rc = libs[name].fnp_spconv_forward(P(x.data_ptr()), I(_l.dtype_code(x)), I(n_in), P(w.data_ptr()), P(rb.nbr.data_ptr()), I(rb.nbr.shape[1]), I(3),
                                           P(nd.data_ptr()), I(cap), P(outs[name].data_ptr()), I(_l.dtype_code(outs[name])), P(sc.data_ptr()), P(sh.data_ptr()),
                                           P(None), I(1), I(0), I(128), I(128), stream)
        assert rc == 0, (name, rc)

    for name in libs:
        for _ in range(3):
            launch(name)
    torch.cuda.synchronize()
    equal = {name: bool(torch.equal(outs[name][:n], outs["main"][:n])) for name in libs}
    times = {name: [] for name in libs}
    for rnd in range(args.warm_rounds + args.rounds):
        for name in libs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                launch(name)
            e1.record()
            torch.cuda.synchronize()
            if rnd >= args.warm_rounds:
                times[name].append(e0.elapsed_time(e1) / args.reps)
    print(json.dumps({"layer": "conv_out", "out": args.out, "rows": n, "cap": cap, "scenes": B,
                      "ms_per_launch_median": {k: round(float(np.median(v)), 4) for k, v in times.items()},
                      "ms_all_rounds": {k: [round(t, 4) for t in v] for k, v in times.items()}, "bit_identical_to_main": equal}), flush=True)
