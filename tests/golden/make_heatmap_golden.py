#!/usr/bin/env python3
"""Golden vectors for the dense heatmap targets and the heatmap loss of TransFusionHead by RUNNING THE REFERENCE:
pcdet/models/dense_heads/transfusion_head.py (TransFusionHead.get_targets_single, called unbound on a stand-in self, per scene
as get_targets does), pcdet/models/model_utils/centernet_utils.py (gaussian_radius, gaussian2D, draw_gaussian_to_heatmap),
pcdet/utils/loss_utils.py (GaussianFocalLoss) and pcdet/models/model_utils/transfusion_utils.py (clip_sigmoid), all on the CPU.

Runs in the build container only (needs the reference).  The reference modules are imported from where they lie.  The
(class, cx, cy, r) of every box is what the method itself hands to draw_gaussian_to_heatmap: the call is recorded on its way
through.  Output: tests/golden/heatmap_golden.npz (arrays only); tests/ref_heatmap.py reads the cases back."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("FNP_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_heatmap as RH  # noqa: E402  (the case table and the input generators only)

NUM_PROPOSALS = 200


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

    for name in ("SharedArray", "cv2", "easydict", "spconv", "spconv.pytorch", "cumm", "cumm.tensorview", "numba", "tqdm",
                 "matplotlib", "matplotlib.pyplot", "torchvision", "torchvision.utils", "torchvision.ops"):
        stub(name).__getattr__ = lambda k: _Any()  # type: ignore
    p = os.path.join(REF, "pcdet")
    shell("pcdet", p)
    shell("pcdet.utils", os.path.join(p, "utils"))
    shell("pcdet.ops", os.path.join(p, "ops"))
    shell("pcdet.ops.iou3d_nms", os.path.join(p, "ops", "iou3d_nms"))
    shell("pcdet.models", os.path.join(p, "models"))
    shell("pcdet.models.dense_heads", os.path.join(p, "models", "dense_heads"))
    shell("pcdet.models.model_utils", os.path.join(p, "models", "model_utils"))
    shell("pcdet.models.dense_heads.target_assigner", os.path.join(p, "models", "dense_heads", "target_assigner"))
    sys.modules["pcdet.ops.iou3d_nms"].iou3d_nms_utils = stub("pcdet.ops.iou3d_nms.iou3d_nms_utils")
    stub("pcdet.models.dense_heads.target_assigner.hungarian_assigner", HungarianAssigner3D=lambda *a, **k: None)
    stub("pcdet.models.dense_heads.pseudo_processor", PseudoProcessor=object)
    stub("pcdet.models.model_utils.basic_block_2d", BasicBlock2D=object)
    stub("pcdet.utils.box_utils")
    th = importlib.import_module("pcdet.models.dense_heads.transfusion_head")
    cu = importlib.import_module("pcdet.models.model_utils.centernet_utils")
    lu = importlib.import_module("pcdet.utils.loss_utils")
    tu = importlib.import_module("pcdet.models.model_utils.transfusion_utils")
    return th, cu, lu, tu


class AttrDict(dict):
    __getattr__ = dict.__getitem__


def stand_in(cfg):
    """the attributes get_targets_single reads from self"""
    C = cfg["num_classes"]
    s = types.SimpleNamespace()
    s.decode_bbox = lambda *a, **k: [{"pred_boxes": torch.zeros(NUM_PROPOSALS, 9)}]
    s.bbox_assigner = types.SimpleNamespace(assign=lambda *a, **k: (torch.zeros(NUM_PROPOSALS, dtype=torch.long), torch.zeros(NUM_PROPOSALS)))
    s.encode_bbox = lambda b: torch.zeros(b.shape[0], 10)
    s.code_size = 10
    s.num_classes = C
    s.use_pseudo = bool(cfg["unknown_labels"])
    s.pseudo_processor = types.SimpleNamespace(unknown_labels=list(cfg["unknown_labels"]))
    s.model_cfg = AttrDict(TARGET_ASSIGNER_CONFIG=AttrDict(GAUSSIAN_OVERLAP=RH.OVERLAP, MIN_RADIUS=RH.MIN_RADIUS, UNK_RADIUS_MULT=cfg["unk_mult"]))
    s.grid_size = np.array(cfg["grid_size"])
    s.feature_map_stride = RH.STRIDE
    s.voxel_size = list(RH.VOXEL_SIZE)
    s.point_cloud_range = np.array(cfg["point_cloud_range"], dtype=np.float32)
    return s


def preds(C):
    return {k: torch.zeros(1, n, NUM_PROPOSALS) for k, n in (("heatmap", C), ("center", 2), ("height", 1), ("dim", 3), ("rot", 2), ("vel", 2))}


def run_scene(th, cfg, rows, draw=True):
    """one scene (M, 10) through get_targets_single -> heatmap (C, H, W), params (M, 4)"""
    C = cfg["num_classes"]
    log = []
    orig = th.centernet_utils.draw_gaussian_to_heatmap

    def recorder(plane, center, radius, *a, **k):
        log.append((plane.storage_offset() // (plane.shape[0] * plane.shape[1]), int(center[0]), int(center[1]), int(radius)))
        return orig(plane, center, radius, *a, **k) if draw else plane

    valid = np.nonzero((rows[:, 3] > 0) & (rows[:, 4] > 0))[0]      # get_targets' "filter empty boxes"
    t = torch.from_numpy(rows[valid])
    th.centernet_utils.draw_gaussian_to_heatmap = recorder
    try:
        out = th.TransFusionHead.get_targets_single(stand_in(cfg), t[:, :-1], t[:, -1].long() - 1, preds(C))
    finally:
        th.centernet_utils.draw_gaussian_to_heatmap = orig
    assert len(log) == valid.size, (len(log), valid.size)
    params = np.zeros((rows.shape[0], 4), np.int32)
    params[:, 0] = -1
    params[valid] = np.array(log, np.int32).reshape(-1, 4)
    return out[6][0].numpy(), params


def main():
    torch.set_num_threads(1)
    th, cu, lu, tu = load_reference()
    save = {}
    for name, cfg in RH.CASES.items():
        boxes = RH.case_boxes(name)
        hms, pars = zip(*(run_scene(th, cfg, boxes[b]) for b in range(boxes.shape[0])))
        save[name + "_boxes"], save[name + "_heatmap"], save[name + "_params"] = boxes, np.stack(hms), np.stack(pars)
        print(name, boxes.shape, "ones", int((save[name + "_heatmap"] == 1).sum()), "max r", int(save[name + "_params"][..., 3].max(initial=0)))
    # 20 000 boxes through the method's own parameter lines, nothing drawn
    many = RH.many_boxes()
    _, p = run_scene(th, RH.MANY_CFG, many, draw=False)
    assert (p[:, 0] >= 0).all()
    save["many_boxes"], save["many_params"] = many, p
    # the weights of radii 0..40 as draw_gaussian_to_heatmap makes them: one quadrant each (the table is symmetric), concatenated
    quads = []
    for r in range(41):
        d = 2 * r + 1
        g = torch.from_numpy(cu.gaussian2D((d, d), sigma=d / 6)).float().numpy()
        assert np.array_equal(g, g[::-1]) and np.array_equal(g, g.T)
        quads.append(g[r:, r:].ravel())
    save["weights_quadrants"] = np.concatenate(quads)
    # loss: the reference's classes in f64 and in f32, per element, and the gradient of their plain sum
    rng = np.random.default_rng(11)
    x, t = RH.make_logits(rng, RH.LOSS_SHAPE), RH.make_targets(rng, RH.LOSS_SHAPE)
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        xx = torch.tensor(x, dtype=dt, requires_grad=True)
        e = lu.GaussianFocalLoss()(tu.clip_sigmoid(xx.clone()), torch.tensor(t, dtype=dt))
        e.sum().backward()
        save["loss_elem_" + tag], save["loss_grad_" + tag] = e.detach().numpy(), xx.grad.numpy()
    save["loss_x"], save["loss_t"] = x, t
    path = os.path.join(HERE, "heatmap_golden.npz")
    np.savez_compressed(path, **save)
    print(len(save), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
