#!/usr/bin/env python3
"""tests/golden/iou3d_ref_gpu.npz: what the reference's own iou3d kernels (pcdet/ops/iou3d_nms/src/iou3d_nms_kernel.cu, compiled
by hipcc into oracle/_ref/libref_iou3d_gpu.so by `make -C oracle ref`) return on an MI355X for the inputs of
tests/test_gpu_ops.py::test_rotated_iou_bit_exact_vs_reference_kernels and ::test_nms_keep_lists_bit_exact (the `rng` fixture's
stream, seed 1234, fresh for every test case).

Needs a GPU and oracle/_ref.  The fixture is data: a SHA-256 of each input, the overlap / IoU matrices and the u64 suppression
masks of the NMS kernels.  usage: make_iou3d_ref_golden.py [output .npz, default tests/golden/iou3d_ref_gpu.npz]"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref_loader  # noqa: E402
import test_gpu_ops as G  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else G.IOU_GOLD
    ref = ref_loader.iou3d_gpu_lib()
    assert ref is not None, "oracle/_ref/libref_iou3d_gpu.so missing: run `make -C oracle ref` where the reference tree is"
    dev = torch.device("cuda", 0)
    fix = {}
    A, Bx = G.iou_inputs(np.random.default_rng(1234))
    fix["iou_inputs_sha256"] = np.array(G._sha(A, Bx))
    for k, t in G.iou_reference(ref, torch.from_numpy(A).to(dev), torch.from_numpy(Bx).to(dev)).items():
        fix[k] = t.cpu().numpy()
    for rotated in (False, True):
        for n in G.NMS_SIZES:
            boxes, scores = G.nms_inputs(np.random.default_rng(1234), n)
            d_boxes, d_scores = torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev)
            sb = d_boxes[torch.sort(d_scores, descending=True)[1]].contiguous()
            tag = f"nms_{'rotated' if rotated else 'normal'}_{n}"
            fix[f"{tag}_inputs_sha256"] = np.array(G._sha(sb.cpu().numpy()))
            for thresh in G.NMS_THRESHOLDS:
                fix[f"{tag}_mask_{thresh}"] = G.nms_reference_mask(ref, sb, thresh, rotated)
    np.savez_compressed(out, **fix)
    print(out, os.path.getsize(out), "bytes,", len(fix), "arrays")


if __name__ == "__main__":
    main()
