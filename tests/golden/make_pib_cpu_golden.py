#!/usr/bin/env python3
"""tests/golden/pib_cpu_ref.npz: what the reference's own points_in_boxes_cpu (pcdet/ops/roiaware_pool3d/src/
roiaware_pool3d.cpp:143-168, built into oracle/_ref by `make -C oracle ref`) returns for the four inputs of
tests/test_oracle_ops.py::test_points_in_boxes_dense_matches_reference_cpp (the `rng` fixture's stream, seed 1234).

Needs the reference tree at build time.  The fixture is data: per input pair a SHA-256 of the inputs and the (17, 20000)
0/1 point-in-box mask, bit-packed (np.packbits, row-major)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref_loader  # noqa: E402
from test_oracle_ops import PIB_GOLD, pib_inputs_sha256, pib_trials  # noqa: E402


def main():
    ref = ref_loader.roiaware_cpu_module()
    assert ref is not None, "oracle/_ref/roiaware_pool3d_ref.so missing: run `make -C oracle ref` where the reference tree is"
    fix = {}
    for trial, (boxes, pts) in enumerate(pib_trials(np.random.default_rng(1234))):
        out = torch.zeros((boxes.shape[0], pts.shape[0]), dtype=torch.int32)
        ref.points_in_boxes_cpu(torch.from_numpy(boxes), torch.from_numpy(pts), out)
        m = out.numpy()
        assert set(np.unique(m).tolist()) <= {0, 1}
        fix[f"inputs_sha256_{trial}"] = np.array(pib_inputs_sha256(boxes, pts))
        fix[f"mask_{trial}"] = np.packbits(m.astype(np.uint8).ravel())
        print(f"trial {trial}: {int(m.sum())} (box, point) pairs inside")
    np.savez_compressed(PIB_GOLD, **fix)
    print(PIB_GOLD, os.path.getsize(PIB_GOLD), "bytes")


if __name__ == "__main__":
    main()
