#!/usr/bin/env python3
"""Golden vectors for gt_sampling by RUNNING THE REFERENCE's pcdet/datasets/augmentor/data_augmentor.py (DataAugmentor.forward:
gt_sampling, then the world ops where the case lists them) and its database_sampler.py (DataBaseSampler alone) on the seeded
databases and scenes of tests/gt_sampling_scenario.py.

Runs in the build container only (needs the reference tree, FNP_REFERENCE, and oracle/_ref built by oracle/Makefile).  The
reference modules are imported from where they lie, under shell packages, with the stubs of make_augment_golden.py.  The cut
is the reference's own points_in_boxes_cpu (oracle/_ref/roiaware_pool3d_ref.so, oracle.ref_loader.roiaware_cpu_module()) under
its own roiaware_pool3d_utils.py; the oracle's rotated BEV IoU stands in for boxes_bev_iou_cpu (as in make_pseudo_golden.py).
Output: tests/golden/gt_sampling_golden.npz (arrays only): db_sha256/<db> of every database written, and per case and call
<case>/<call>/{points,gt_boxes,gt_names,next_draw} after the augmentor and sampler/<case>/<call>/{points,gt_boxes,gt_names,
next_draw} after a DataBaseSampler alone (next_draw: the np.random.random() that would come next)."""
import importlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import gt_sampling_scenario as SC  # noqa: E402
import make_augment_golden as MA  # noqa: E402
from make_pseudo_golden import boxes_bev_iou_cpu  # noqa: E402
from oracle import ref_loader  # noqa: E402

SAMPLER_CASES = ("transfusion", "no_gt", "extra_width", "faces")


def load_reference():
    MA.load_reference()    # shells, stubs; the two ops modules are stubs until filled in here
    cuda = ref_loader.roiaware_cpu_module()
    assert cuda is not None, "oracle/_ref/roiaware_pool3d_ref.so is missing: make -C oracle ref"
    sys.modules["pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda"] = cuda
    sys.modules["pcdet.ops.roiaware_pool3d"].roiaware_pool3d_cuda = cuda
    del sys.modules["pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils"]
    pib = importlib.import_module("pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils")
    sys.modules["pcdet.ops.roiaware_pool3d"].roiaware_pool3d_utils = pib
    sys.modules["pcdet.ops.iou3d_nms.iou3d_nms_utils"].boxes_bev_iou_cpu = boxes_bev_iou_cpu
    for m in ("pcdet.utils.box_utils", "pcdet.datasets.augmentor.database_sampler", "pcdet.datasets.augmentor.data_augmentor"):
        sys.modules.pop(m, None)
        pkg, name = m.rsplit(".", 1)
        sys.modules[pkg].__dict__.pop(name, None)
    ds = importlib.import_module("pcdet.datasets.augmentor.database_sampler")
    da = importlib.import_module("pcdet.datasets.augmentor.data_augmentor")
    assert ds.box_utils.roiaware_pool3d_utils is pib
    return da, ds


def next_draw():
    st = np.random.get_state()
    v = np.random.random()
    np.random.set_state(st)
    return np.float64(v)


def record(save, key, out):
    save[f"{key}/points"] = np.asarray(out["points"])
    save[f"{key}/gt_boxes"] = np.asarray(out["gt_boxes"])
    save[f"{key}/gt_names"] = np.asarray(out["gt_names"]).astype(str)
    save[f"{key}/next_draw"] = next_draw()


def main():
    from pathlib import Path

    da, ds = load_reference()
    save = {}
    with tempfile.TemporaryDirectory() as root:
        for db in SC.DATABASES:
            save[f"db_sha256/{db}"] = np.array(SC.write_database(root, db))
        for case, (calls, _) in SC.CASES.items():
            np.random.seed(SC.seed_of(case))
            aug = da.DataAugmentor(Path(root), SC.augmentor_config(case), SC.CLASS_NAMES)
            for call in range(calls):
                d = SC.make_scene(case, call)
                if case == "faces":
                    d = SC.add_face_points(d, root)
                record(save, f"{case}/{call}", aug.forward(d))
            if case not in SAMPLER_CASES:
                continue
            np.random.seed(SC.seed_of(case))
            sampler = ds.DataBaseSampler(Path(root), SC.sampler_config(case), SC.CLASS_NAMES)
            for call in range(calls):
                d = SC.make_scene(case, call)
                if case == "faces":
                    d = SC.add_face_points(d, root)
                record(save, f"sampler/{case}/{call}", sampler(d))
    np.savez_compressed(os.path.join(HERE, "gt_sampling_golden.npz"), **save)
    print(len(save), "arrays;", sum(v.nbytes for v in save.values()), "bytes;",
          os.path.getsize(os.path.join(HERE, "gt_sampling_golden.npz")), "bytes compressed")


if __name__ == "__main__":
    main()
