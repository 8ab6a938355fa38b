#!/usr/bin/env python3
"""Golden vectors for the pseudo-label entries of DataAugmentor (load_frustum_pseudos, load_selftrain_pseudos,
unknowns_copy_paste) by RUNNING THE REFERENCE's pcdet/datasets/augmentor/data_augmentor.py with its pseudo_loader.py and
database_sampler.py over the sequences of tests/pseudo_augment_scenario.py (the copy-paste queue carries state from frame to
frame, so every case is one augmentor over all frames).

Runs in the build container only (needs the reference tree, FNP_REFERENCE, and oracle/_ref built by oracle/Makefile).  The
reference modules are imported as make_gt_sampling_golden.py imports them, with the real pseudo_loader.py in place of the
stub and the oracle's rotated BEV IoU standing in for boxes_bev_iou_cpu (as in make_pseudo_golden.py).
Output: tests/golden/pseudo_augment_golden.npz (arrays only): db_sha256/<db>, per case and frame
<case>/<frame>/{points,gt_boxes,gt_names,pseudo_boxes,pseudo_samples_mask,next_draw} after DataAugmentor.forward, and
<case>/queue_sizes, the per-class queue lengths after the sequence (unknown class labels in order)."""
import importlib
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import make_gt_sampling_golden as MG  # noqa: E402
import pseudo_augment_scenario as SC  # noqa: E402


def load_reference():
    MG.load_reference()
    for m in ("pcdet.datasets.augmentor.pseudo_loader", "pcdet.datasets.augmentor.data_augmentor"):
        sys.modules.pop(m, None)
        pkg, name = m.rsplit(".", 1)
        sys.modules[pkg].__dict__.pop(name, None)
    pl = importlib.import_module("pcdet.datasets.augmentor.pseudo_loader")
    da = importlib.import_module("pcdet.datasets.augmentor.data_augmentor")
    assert da.PseudoLoader is pl.PseudoLoader
    return da


def main():
    _load = torch.load     # the reference predates torch's weights_only default
    torch.load = lambda *a, **k: _load(*a, **{**k, "weights_only": k.get("weights_only", False)})
    da = load_reference()
    save = {}
    seen = {"copy box over a sampled box": False, "pasted row inside a cut box": False}
    with tempfile.TemporaryDirectory() as root, tempfile.TemporaryDirectory() as fr, tempfile.TemporaryDirectory() as st:
        for db, sha in SC.write_databases(root).items():
            save[f"db_sha256/{db}"] = np.array(sha)
        frames = SC.make_frames(fr, st)
        for case in SC.CASES:
            np.random.seed(SC.seed_of(case))
            aug = da.DataAugmentor(Path(root), SC.augmentor_config(case, fr, st), SC.CLASS_NAMES)
            log = SC.trace(aug)
            for k, frame in enumerate(frames):
                out = aug.forward(SC.data_dict(frame))
                key = f"{case}/{k}"
                MG.record(save, key, out)
                save[f"{key}/pseudo_boxes"] = np.asarray(out["pseudo_boxes"])
                save[f"{key}/pseudo_samples_mask"] = np.asarray(out["pseudo_samples_mask"], bool)
                assert "pseudo_scores" not in out
            q = aug.pseudo_loader.sampler.unknown_queue
            save[f"{case}/queue_sizes"] = np.array([len(q[l]) for l in aug.pseudo_loader.unknown_class_labels], np.int64)
            if case == "overlap":
                for e in log:
                    a, b = SC.overlaps(e)
                    seen["copy box over a sampled box"] |= a
                    seen["pasted row inside a cut box"] |= b
    assert all(seen.values()), seen
    assert sum(int(v.sum()) for k, v in save.items() if k.endswith("pseudo_samples_mask")) > 20
    np.savez_compressed(os.path.join(HERE, "pseudo_augment_golden.npz"), **save)
    print(len(save), "arrays;", os.path.getsize(os.path.join(HERE, "pseudo_augment_golden.npz")), "bytes compressed")


if __name__ == "__main__":
    main()
