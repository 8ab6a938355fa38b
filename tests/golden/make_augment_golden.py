#!/usr/bin/env python3
"""Golden vectors for the world augmentations, the range mask and the point shuffle by RUNNING THE REFERENCE's
pcdet/datasets/augmentor/data_augmentor.py (DataAugmentor.forward over augmentor_utils.py) and
pcdet/datasets/processor/data_processor.py (DataProcessor: mask_points_and_boxes_outside_range, shuffle_points) on the
seeded synthetic scenes of tests/augment_scenario.py.

Runs in the build container only (needs the reference tree, FNP_REFERENCE).  The reference modules are imported from where
they lie, under shell packages; the modules they import that the augmentations never call (SharedArray, skimage,
torchvision, the KITTI helpers, the compiled ops) are stubs.  Output: tests/golden/augment_golden.npz (arrays only):
per case <case>/<scene>/{points,gt_boxes,pseudo_boxes,flip_x,flip_y,noise_rot,noise_scale,noise_translate} after the
augmentor, <case>/<scene>/{perm,final} after the processor (perm: the np.random.permutation the shuffle drew)."""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("FNP_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import augment_scenario as SC  # noqa: E402


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def shell(name, path):
    m = types.ModuleType(name)
    m.__path__ = [path]
    sys.modules[name] = m
    return m


def load_reference():
    class _Any:
        def __getattr__(self, k):
            return _Any()

        def __call__(self, *a, **k):
            return _Any()

    def _attr(k):
        if k.startswith("__"):
            raise AttributeError(k)
        return _Any()

    for name in ("SharedArray", "skimage", "skimage.io", "skimage.transform", "torchvision", "cv2", "numba", "tqdm",
                 "spconv", "spconv.pytorch", "cumm", "cumm.tensorview"):
        stub(name).__getattr__ = _attr  # type: ignore
    p = os.path.join(REF, "pcdet")
    shell("pcdet", p)
    shell("pcdet.utils", os.path.join(p, "utils"))
    shell("pcdet.ops", os.path.join(p, "ops"))
    shell("pcdet.ops.iou3d_nms", os.path.join(p, "ops", "iou3d_nms"))
    shell("pcdet.ops.roiaware_pool3d", os.path.join(p, "ops", "roiaware_pool3d"))
    shell("pcdet.datasets", os.path.join(p, "datasets"))
    shell("pcdet.datasets.kitti", os.path.join(p, "datasets", "kitti"))
    shell("pcdet.datasets.kitti.kitti_object_eval_python", os.path.join(p, "datasets", "kitti", "kitti_object_eval_python"))
    shell("pcdet.datasets.augmentor", os.path.join(p, "datasets", "augmentor"))
    shell("pcdet.datasets.processor", os.path.join(p, "datasets", "processor"))
    sys.modules["pcdet.ops.iou3d_nms"].iou3d_nms_utils = stub("pcdet.ops.iou3d_nms.iou3d_nms_utils")
    sys.modules["pcdet.ops.roiaware_pool3d"].roiaware_pool3d_utils = stub("pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils")
    stub("pcdet.datasets.kitti.kitti_object_eval_python.kitti_common")
    stub("pcdet.utils.calibration_kitti")
    stub("pcdet.datasets.augmentor.pseudo_loader", PseudoLoader=object)
    da = importlib.import_module("pcdet.datasets.augmentor.data_augmentor")
    dp = importlib.import_module("pcdet.datasets.processor.data_processor")
    return da, dp


def main():
    da, dp = load_reference()
    drawn = []
    _perm = np.random.permutation

    def permutation(n):   # record what shuffle_points draws
        p = _perm(n)
        drawn.append(np.asarray(p))
        return p

    np.random.permutation = permutation
    save = {}
    for case in SC.CASES:
        aug_cfg = SC.augmentor_config(case, SC.EDict)
        proc = dp.DataProcessor(SC.processor_config(SC.EDict), np.array(SC.POINT_CLOUD_RANGE, np.float32), training=True,
                                num_point_features=5)
        for s in range(SC.NUM_SCENES):
            d = SC.make_scene(case, s)
            np.random.seed(SC.seed_of(case, s))
            aug = da.DataAugmentor(None, aug_cfg, SC.CLASS_NAMES)
            out = aug.forward(d)
            key = f"{case}/{s}"
            for k in SC.AUG_KEYS:
                if k in out:
                    save[f"{key}/{k}"] = np.asarray(out[k])
            drawn.clear()
            out = proc.forward(out)
            assert len(drawn) == 1
            save[f"{key}/perm"] = drawn[0].astype(np.int64)
            save[f"{key}/final"] = out["points"]
            save[f"{key}/final_gt_boxes"] = out["gt_boxes"]
    np.random.permutation = _perm
    np.savez_compressed(os.path.join(HERE, "augment_golden.npz"), **save)
    print(len(save), "arrays;", sum(v.nbytes for v in save.values()), "bytes")


if __name__ == "__main__":
    main()
