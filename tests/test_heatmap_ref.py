"""tests/ref_heatmap.py and the plain mirrors, held to the reference's own output (tests/golden/heatmap_golden.npz, made by
tests/golden/make_heatmap_golden.py from TransFusionHead.get_targets_single, centernet_utils, GaussianFocalLoss and clip_sigmoid
run on the CPU).  No GPU."""
import os

import numpy as np
import pytest
import torch

import ref_heatmap as RH

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heatmap_golden.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(RH.CASES))
def test_restatement_equals_reference_targets(gold, name):
    cfg = RH.CASES[name]
    hm, num_pos, params = RH.targets(gold[name + "_boxes"], grid_size=cfg["grid_size"], **RH.case_kwargs(name))
    assert np.array_equal(params, gold[name + "_params"])
    assert hm.shape == gold[name + "_heatmap"].shape
    assert np.array_equal(hm, gold[name + "_heatmap"])
    assert num_pos == int((gold[name + "_heatmap"] == 1).sum())


def test_fixture_shapes_cover_the_cases(gold):
    assert gold["a_heatmap"].shape == (2, 10, 200, 176)                         # non-square: H along y, W along x
    assert ((gold["a_params"][..., 0] < 0).sum(1) > 0).all()                     # padded rows between valid ones
    assert (gold["d_params"][0, :, 0] == 0).sum() > 2 * 256                      # one class, more than one chunk of 256
    b = gold["b_params"][0]
    assert b[:, 1].min() < -8 and b[:, 1].max() > 179 + 8 and b[:, 2].min() < -8 and b[:, 2].max() > 179 + 8
    assert (b[-2, 1], b[-2, 2]) == (0, 0) and gold["b_boxes"][0, -2, 0] < RH.CASES["b"]["point_cloud_range"][0]
    assert gold["e_heatmap"].shape[1] == 1 and gold["f0_boxes"].shape[1] == 0 and not gold["f1_heatmap"].any()
    for name, mult in (("c1", 1.5), ("c2", 2.0)):                                # unknown labels really grew their radius
        lab = gold[name + "_boxes"][0, :, -1].astype(int)
        unk = np.isin(lab, RH.CASES[name]["unknown_labels"])
        plain = RH.box_params(gold[name + "_boxes"], **{**RH.case_kwargs(name), "unknown_labels": ()})[0, :, 3]
        assert unk.any() and np.array_equal(gold[name + "_params"][0, unk, 3], (plain[unk] * mult).astype(int))


def test_restatement_equals_reference_on_20000_boxes(gold):
    boxes = gold["many_boxes"]
    assert boxes.shape[0] == 20000
    assert np.array_equal(RH.box_params(boxes, **RH.case_kwargs("many")), gold["many_params"])
    assert gold["many_params"][:, 3].max() >= 10 and gold["many_params"][:, 3].min() == RH.MIN_RADIUS


def test_restated_weights_equal_gaussian2D(gold):
    off = RH.quadrant_offsets()
    for r in range(41):
        want = gold["weights_quadrants"][off[r]:off[r + 1]].reshape(r + 1, r + 1)
        assert np.array_equal(RH.gaussian_f32(r)[r:, r:], want), r


def test_restated_f64_loss_equals_reference_f64(gold):
    """at the reference's own f64 constants (clamp 1e-4 / 1 - 1e-4, eps 1e-12) to 1e-12 relative; the yardstick's constants (the
    f32-rounded clamp, no eps) move the result only on clamped elements and by the 1e-12 inside the logarithms"""
    x, t = gold["loss_x"], gold["loss_t"]
    r = RH.loss64(x, t, lo=1e-4, hi=1 - 1e-4, eps=1e-12)
    for got, want in ((r["T"], gold["loss_elem_f64"]), (r["G"], gold["loss_grad_f64"])):
        assert np.array_equal(got == 0, want == 0)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        nz = want != 0
        assert (np.abs(got - want)[nz] / np.abs(want)[nz]).max() <= 1e-12
    y = RH.loss64(x, t)
    clamped = ~y["inside"]
    assert clamped.any() and (~clamped).any()
    # inside the clamp the two differ by eps alone: |d log| <= eps / min(p, q)
    rel = np.abs(y["T"] - r["T"])[~clamped] / np.abs(r["T"])[~clamped]
    assert rel.max() <= 1e-12 / 1e-4 * 1.01
    # on clamped elements by the constants' rounding: f32(1e-4) - 1e-4 and f32(1 - 1e-4) - (1 - 1e-4), through dT/dp
    dlo, dhi = abs(RH.CLAMP_LO - 1e-4), abs(RH.CLAMP_HI - (1 - 1e-4))
    p, q, w = r["p"], r["q"], r["w"]
    dTdp = np.where(r["pos"], q * q / p + 2 * q * np.abs(r["lp"]), w * (p * p / q + 2 * p * np.abs(r["lq"])))
    assert (np.abs(y["T"] - r["T"])[clamped] <= (dTdp * max(dlo, dhi))[clamped] * 1.01 + 1e-12 * np.abs(r["T"])[clamped] / 1e-4).all()


def test_reference_f32_lies_inside_the_bounds(gold):
    """the bounds are ones the reference's own f32 run meets"""
    x, t = gold["loss_x"], gold["loss_t"]
    assert x.shape == RH.LOSS_SHAPE and (t == 1).sum() > 10 and (t == 0).sum() > 100 and ((t > 0) & (t < 1)).sum() > 100
    assert x.min() < -11 and x.max() > 11 and (np.abs(np.abs(x) - np.log(1 / 1e-4 - 1)) >= 1e-3).all()
    r = RH.loss64(x, t)
    ratio_T = np.abs(gold["loss_elem_f32"] - r["T"]) / RH.tol_T(r)
    print("reference f32 loss / bound:", ratio_T.max(), "at k = a = 4:", (np.abs(gold["loss_elem_f32"] - r["T"]) / RH.tol_T(r, 4, 4)).max())
    assert ratio_T.max() <= 1
    inside = r["inside"]
    assert np.array_equal(gold["loss_grad_f32"] == 0, ~inside)            # exactly zero outside the clamp, nowhere else
    ratio_G = np.abs(gold["loss_grad_f32"] - r["G"])[inside] / RH.tol_G(r)[inside]
    print("reference f32 gradient / bound:", ratio_G.max())
    assert ratio_G.max() <= 1


def test_plain_mirrors_equal_reference(gold):
    from findnpropagate_amd.model_utils import centernet_utils as CU
    from findnpropagate_amd.model_utils.transfusion_utils import clip_sigmoid
    from findnpropagate_amd.utils.loss_utils import GaussianFocalLoss, heatmap_loss

    # gaussian_radius on one-element tensors as the head calls it, and the drawing, on case c2 (unknown labels, multiplier 2)
    name = "c2"
    cfg, boxes, want = RH.CASES[name], torch.from_numpy(gold[name + "_boxes"][0]), gold[name + "_params"][0]
    hm = torch.zeros(gold[name + "_heatmap"].shape[1:])
    for i in range(boxes.shape[0]):
        width = boxes[i][3] / RH.VOXEL_SIZE[0] / RH.STRIDE
        length = boxes[i][4] / RH.VOXEL_SIZE[1] / RH.STRIDE
        radius = max(RH.MIN_RADIUS, int(CU.gaussian_radius(length.view(-1), width.view(-1), RH.OVERLAP)[0]))
        if int(boxes[i][-1]) in cfg["unknown_labels"]:
            radius = int(radius * cfg["unk_mult"])
        assert radius == want[i, 3]
        CU.draw_gaussian_to_heatmap(hm[want[i, 0]], want[i, 1:3], radius)
    assert np.array_equal(hm.numpy(), gold[name + "_heatmap"][0])
    # the edge case through the mirror's clipping
    hm = torch.zeros(gold["b_heatmap"].shape[1:])
    for c, x, y, r in gold["b_params"][0].tolist():
        CU.draw_gaussian_to_heatmap(hm[c], (x, y), r)
    assert np.array_equal(hm.numpy(), gold["b_heatmap"][0])
    off = RH.quadrant_offsets()
    assert np.array_equal(CU.gaussian2D((81, 81), sigma=81 / 6).astype(np.float32)[40:, 40:].ravel(), gold["weights_quadrants"][off[40]:off[41]])
    # loss classes, f32 and f64, per element and gradient
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        x = torch.tensor(gold["loss_x"], dtype=dt, requires_grad=True)
        logits = x.clone()
        e = GaussianFocalLoss()(clip_sigmoid(logits), torch.tensor(gold["loss_t"], dtype=dt))
        e.sum().backward()
        assert np.array_equal(e.detach().numpy(), gold["loss_elem_" + tag])
        assert np.array_equal(x.grad.numpy(), gold["loss_grad_" + tag])
        assert torch.equal(logits.detach(), x.detach().sigmoid())            # the in-place sigmoid of the reference
    # the composition on the CPU: the sum over max(num_pos, 1), logits left alone
    x = torch.tensor(gold["loss_x"])
    keep = x.clone()
    t = torch.tensor(gold["loss_t"])
    n = int((gold["loss_t"] == 1).sum())
    want = torch.tensor(gold["loss_elem_f32"]).sum() / n
    assert torch.equal(heatmap_loss(x, t), want) and torch.equal(heatmap_loss(x, t, torch.tensor([n], dtype=torch.int32)), want)
    assert torch.equal(heatmap_loss(x, torch.zeros_like(t)), GaussianFocalLoss()(clip_sigmoid(x.clone()), torch.zeros_like(t)).sum())
    assert torch.equal(x, keep)


def test_heatmap_targets_parses_the_shipped_config():
    from findnpropagate_amd.dense_heads.transfusion_targets import HeatmapTargets

    shipped = {"FEATURE_MAP_STRIDE": 8, "DATASET": "nuScenes", "GAUSSIAN_OVERLAP": 0.1, "MIN_RADIUS": 2, "UNK_RADIUS_MULT": 1,
               "HUNGARIAN_ASSIGNER": {"cls_cost": {"gamma": 2.0, "alpha": 0.25, "weight": 0.15}, "reg_cost": {"weight": 0.25},
                                      "iou_cost": {"weight": 0.25}}}     # transfusion_lidar.yaml, DENSE_HEAD.TARGET_ASSIGNER_CONFIG

    class Attr(dict):
        __getattr__ = dict.__getitem__

    for cfg in (shipped, Attr(shipped)):
        h = HeatmapTargets(cfg, np.array([1440, 1440, 40]), [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], [0.075, 0.075, 0.2], 10, unknown_labels=[3, 7, 9])
        assert (h.stride, h.overlap, h.min_radius, h.unk_mult) == (8, 0.1, 2, 1.0)
        assert (h.H, h.W, h.num_classes) == (180, 180, 10) and h.unk_mask == (1 << 2) | (1 << 6) | (1 << 8)
    del shipped["UNK_RADIUS_MULT"]
    h = HeatmapTargets(shipped, [1408, 1600, 40], [-52.8, -60.0, -5.0, 52.8, 60.0, 3.0], [0.075, 0.075, 0.2], 10)
    assert (h.H, h.W, h.unk_mult, h.unk_mask) == (200, 176, 1.0, 0)


def test_entry_points_are_declared():
    from findnpropagate_amd import lib

    names = {"fnp_heatmap_box_params", "fnp_heatmap_draw_workspace_bytes", "fnp_heatmap_draw", "fnp_heatmap_loss_workspace_bytes",
             "fnp_heatmap_loss_forward", "fnp_heatmap_loss_backward"}
    assert names <= set(lib.SIGNATURES) and names <= set(lib.header_symbols())
