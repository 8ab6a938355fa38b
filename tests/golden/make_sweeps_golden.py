#!/usr/bin/env python3
"""Golden vectors for multi-sweep assembly by RUNNING THE REFERENCE's pcdet/datasets/nuscenes/nuscenes_dataset.py
(NuScenesDataset.get_sweep and get_lidar_with_sweeps, as they stand) on the seeded samples of tests/sweeps_scenario.py, whose
sweep files are written into a temporary directory first.

Runs in the build container only (needs the reference tree, FNP_REFERENCE).  The reference module is imported from where it
lies, under shell packages; the modules it imports that the two methods never call (DatasetTemplate, the compiled ops,
common_utils, tqdm, pyquaternion, PIL) are stubs, and the methods run on a stand-in object that carries root_path and infos.
Output: tests/golden/sweeps_golden.npz (arrays only, the recorded outputs; the inputs are regenerated from seeds):
  points/<s>            get_lidar_with_sweeps(s, MAX_SWEEPS[s]) after np.random.seed(seed_of(s))
  order/<s>             the sweep indices that call drew
  sweep/<s>/<k>/points, sweep/<s>/<k>/times   get_sweep(infos[s]['sweeps'][k]) for the sweeps of scene 3"""
import importlib
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("FNP_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sweeps_scenario as SC  # noqa: E402


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

    for name in ("tqdm", "pyquaternion", "PIL", "PIL.Image"):
        stub(name).__getattr__ = _attr  # type: ignore
    p = os.path.join(REF, "pcdet")
    shell("pcdet", p)
    shell("pcdet.datasets", os.path.join(p, "datasets"))
    shell("pcdet.datasets.nuscenes", os.path.join(p, "datasets", "nuscenes"))
    shell("pcdet.ops", os.path.join(p, "ops"))
    shell("pcdet.utils", os.path.join(p, "utils"))
    ops = shell("pcdet.ops.roiaware_pool3d", os.path.join(p, "ops", "roiaware_pool3d"))
    ops.roiaware_pool3d_utils = stub("pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils")
    sys.modules["pcdet.utils"].common_utils = stub("pcdet.utils.common_utils")
    stub("pcdet.datasets.dataset", DatasetTemplate=object)
    return importlib.import_module("pcdet.datasets.nuscenes.nuscenes_dataset")


def main():
    ref = load_reference()

    class StandIn:
        get_sweep = ref.NuScenesDataset.get_sweep
        get_lidar_with_sweeps = ref.NuScenesDataset.get_lidar_with_sweeps

    infos, files = SC.make_dataset()
    drawn = []
    _choice = np.random.choice

    def choice(*a, **k):   # record what get_lidar_with_sweeps draws
        r = _choice(*a, **k)
        drawn.append(np.asarray(r))
        return r

    save = {}
    with tempfile.TemporaryDirectory() as tmp:
        SC.write_files(tmp, files)
        ds = StandIn()
        ds.root_path, ds.infos = Path(tmp), infos
        np.random.choice = choice
        try:
            for s in range(SC.NUM_SCENES):
                drawn.clear()
                np.random.seed(SC.seed_of(s))
                save[f"points/{s}"] = ds.get_lidar_with_sweeps(s, max_sweeps=SC.MAX_SWEEPS[s])
                assert len(drawn) == 1
                save[f"order/{s}"] = drawn[0].astype(np.int64)
        finally:
            np.random.choice = _choice
        for k, sw in enumerate(infos[3]["sweeps"]):
            pts, times = ds.get_sweep(sw)
            save[f"sweep/3/{k}/points"] = np.ascontiguousarray(pts)
            save[f"sweep/3/{k}/times"] = np.ascontiguousarray(times)
    for k, v in save.items():
        assert isinstance(v, np.ndarray) and v.dtype != object, k
    np.savez_compressed(os.path.join(HERE, "sweeps_golden.npz"), **save)
    print(len(save), "arrays;", sum(v.nbytes for v in save.values()), "bytes;",
          {s: save[f"points/{s}"].shape for s in range(SC.NUM_SCENES)})


if __name__ == "__main__":
    main()
