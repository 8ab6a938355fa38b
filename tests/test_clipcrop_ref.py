"""The float64 restatement of the CLIP-crop geometry (tests/ref_clipcrop.py) tied to the reference's own run, on the CPU:
the f32 projections recorded from the reference's project_to_camera lie inside the restatement's v +- e, the crop list its
decided pairs imply is the reference's, its bilinear sampling agrees with torch's grid_sample inside the per-element bound,
and every case the GPU tests run (tests/test_gpu_clipcrop.py) decides enough pairs to hold the kernel to something."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_clipcrop as R  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rinv_trans(lidar_aug):
    """What the module passes to the kernel: torch's f32 inverse of the 3 x 3 block, and the translation."""
    a = torch.from_numpy(np.ascontiguousarray(lidar_aug))
    return torch.inverse(a[:3, :3]).contiguous().numpy(), a[:3, 3].contiguous().numpy()


def scenes():
    """(id, boxes, lidar_aug, lidar2image, img_aug, H, W, proj_yxz, crop_pair, crop_rect) of every fixture scene."""
    out = []
    for seed in range(3):
        g = np.load(os.path.join(GOLD, f"clipcrop_seed{seed}.npz"))
        out.append((f"seed{seed}", g["boxes"], g["lidar_aug"], g["lidar2image"], g["img_aug"], 900, 1600, g["proj_yxz"], g["crop_pair"], g["crop_rect"]))
    g = np.load(os.path.join(GOLD, "clipcrop_aug_b2.npz"))
    at = np.concatenate([[0], np.cumsum(g["crops_per_scene"])])
    for b in range(2):
        out.append((f"aug_b2_scene{b}", g[f"boxes{b}"], g["lidar_aug"][b], g["lidar2image"][b], g["img_aug"][b], 256, 704, g[f"proj_yxz{b}"],
                    g["crop_pair"][at[b]:at[b + 1]], g["crop_rect"][at[b]:at[b + 1]]))
    return out


SCENES = scenes()


@pytest.mark.parametrize("scene", SCENES, ids=[s[0] for s in SCENES])
def test_reference_projection_inside_bounds(scene):
    name, boxes, aug, l2i, iaug, H, W, proj, _, _ = scene
    rinv, trans = rinv_trans(aug)
    rx, ry, rz, qz = R.project(boxes, rinv, trans, l2i, iaug)
    keep = (qz[0] - qz[1] > 1e-5) & (qz[0] + qz[1] < 1e5)             # depth in the unclamped range
    got = np.transpose(proj, (1, 0, 2, 3))                            # (N, 6, 8, [row, column, depth])
    assert keep.sum() >= 0.3 * keep.size
    ratio = R.worst_ratio((ry, rx, rz), (got[..., 0], got[..., 1], got[..., 2]), keep)
    print(f"RATIO projection {name}: corners {int(keep.sum())} worst |reference f32 - f64| / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("scene", SCENES, ids=[s[0] for s in SCENES])
def test_crop_list_of_decided_boxes_is_the_references(scene):
    name, boxes, aug, l2i, iaug, H, W, _, pair, rect = scene
    rinv, trans = rinv_trans(aug)
    p = R.plan(boxes, rinv, trans, l2i, iaug, H, W)
    whole = p["decided"].all(1)                                       # boxes all of whose six pairs are decided
    assert whole.sum() >= 0.8 * len(boxes)
    want = R.crop_pairs(p["rect"])
    want = want[whole[want[:, 0]]]
    keep = whole[pair[:, 0]]
    assert np.array_equal(want, pair[keep]), "cameras in image_order, boxes ascending"
    assert np.array_equal(p["rect"][want[:, 0], want[:, 1], :3].astype(np.int64), rect[keep].astype(np.int64))
    # and the reference's other crops are admissible
    for (i, c), r in zip(pair[~keep], rect[~keep]):
        assert R.pair_violation(p, i, c, 1, np.array([r[0], r[1], r[2], 1.0])) is None


def reference_grid(S=224):
    g = F.affine_grid(theta=torch.eye(2, 3).unsqueeze(0), size=[1, 3, S, S], align_corners=False)
    return (g - g.min()) / (g.max() - g.min())                         # (1, S, S, 2) in [0, 1]


@pytest.mark.parametrize("which", ["noise_120x200", "procedural_900x1600"])
def test_bilinear_restatement_against_grid_sample(which, rng):
    if which == "noise_120x200":
        H, W = 120, 200
        images = rng.uniform(0, 1, (6, 3, H, W)).astype(np.float32)
    else:
        H, W = 900, 1600
        images = R.procedural_images(H, W)
    ref = R.SampleRef(images)
    unit01 = reference_grid()
    unit = unit01[0, 0, :, 0].contiguous().numpy()
    assert np.array_equal(unit, unit01[0, :, 0, 1].numpy())
    worst = 0.0
    for k, (x1, y1, side, _) in enumerate(R.sample_rects(H, W)):
        c = k % 6
        grid = unit01.clone()
        grid[..., 0] = (grid[..., 0] * int(side) + int(x1)) / W * 2.0 - 1.0          # (:326-332)
        grid[..., 1] = (grid[..., 1] * int(side) + int(y1)) / H * 2.0 - 1.0
        want = F.grid_sample(torch.from_numpy(images[[c]]), grid, align_corners=False)[0].numpy().astype(np.float64)
        val, bound = ref.crop(c, x1, y1, side, unit)
        err = np.abs(want - val)
        if R.SAMPLE_RECTS[k] == "x1=W":       # past pixel coordinate W + 0.5 every tap is off the image: exactly 0, bound 0
            far = unit.astype(np.float64) * float(side) >= 2.0
            assert far.sum() >= 200 and not bound[:, :, far].any() and not val[:, :, far].any()
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        assert np.all(err <= bound), (which, R.SAMPLE_RECTS[k], float((err / np.maximum(bound, 1e-300)).max()))
    print(f"RATIO bilinear {which}: worst |grid_sample f32 - f64| / bound {worst:.3f}")


@pytest.mark.parametrize("name", [c[0] for c in R.PLAN_CASES])
def test_gpu_plan_cases_decide_enough(name):
    """Coverage conditions of the random GPU cases: an undecided pair is held only to its ranges, so at least 95 % of the pairs that
    may be on an image must be decided; and a case must contain crops and crops that are too small.  (The one-box case has six
    pairs in all, so the counts apply from 42 boxes on; its box is placed where it gives a crop.)"""
    c = R.plan_case(name)
    rinv, trans = rinv_trans(c["lidar_aug"])
    args = (c["boxes"], rinv, trans, c["l2i"], c["iaug"])
    p = R.plan(*args, c["H"], c["W"])
    may = p["mask_hi"]
    share = (p["decided"] & may).sum() / may.sum()
    small = (p["mask_lo"] & (p["side_hi"] < 64)).sum()
    vals = R.project(*args)
    keep = (vals[3][0] - vals[3][1] > 1e-5) & (vals[3][0] + vals[3][1] < 1e5)
    ratio = R.worst_ratio(vals[:3], R.replay_f32(*args), keep)
    print(f"RATIO plan {name}: may be on an image {int(may.sum())} decided {share:.4f} crops {int(p['valid'].sum())} too small {int(small)} "
          f"f32 replay / bound {ratio:.3f}")
    assert share >= 0.95 and ratio <= 1.0
    if len(c["boxes"]) >= 42:
        assert p["valid"].sum() >= 10 and small >= 1
    else:
        assert p["valid"].sum() >= 1


NOT_DYADIC = {"behind", "straddle"}      # depth clamps to 1e-5f there; the restatement itself must decide them


@pytest.mark.parametrize("name", list(R.edge_cases()))
def test_edge_case_expectations(name):
    """The hand-computed rect / mask of the exact cases: every f32 operation of the chain is exact on them (the f32 replay equals the
    f64 value bit for bit), so the expected integers follow from the f64 value with no interval."""
    c = R.edge_cases()[name]
    rinv, trans = rinv_trans(c["lidar_aug"])
    args = (c["boxes"], rinv, trans, c["l2i"], c["iaug"])
    if name in NOT_DYADIC:
        p = R.plan(*args, c["H"], c["W"])
        assert p["decided"].all()
    else:
        vals, rep = R.project(*args), R.replay_f32(*args)
        for (v, _), r in zip(vals[:3], rep):
            assert np.array_equal(r.astype(np.float64), v)
        p = R.plan(*args, c["H"], c["W"], exact=True)
    mask, rect = c["expect"]
    assert np.all(p["mask"] == mask) and np.all(p["rect"] == np.array(rect, np.float32))
