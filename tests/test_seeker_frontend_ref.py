"""The plain restatement of the Box Seeker's per-frustum front end in tests/seeker_parity.py (selection, depth quantiles,
frustum corners, per-candidate counts, choice) — what tests/test_gpu_boxseeker_batches.py holds the kernel to on frustums of
tens of thousands of points, where the full oracle is too slow — is itself held
  * to the reference's recording: the corners its get_geometry_at_image_coords returned for every frustum of two fixture scenes
    (tests/golden/boxseeker_seed*.npz, one with a lidar augmentation), fed the oracle's own point selection;
  * to planted defects, each of which a check must report.
CPU only."""
import os

import numpy as np
import pytest

import seeker_parity as SP
from findnpropagate_amd import synthetic as syn

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARAMS = {"lq": 0.0, "uq": 0.25, "cq": 1.0, "clamp_bottom": 0, "score_thr": 0.45, "nms_2d": 0.4}
DEFAULT_Q = {"lq": 0.336, "uq": 0.356, "cq": 0.46, "clamp_bottom": 0}      # the reference's constructor defaults (:144-147)


@pytest.mark.parametrize("seed", [0, 3])
def test_restated_frustum_reproduces_the_recorded_corners(seed):
    from oracle import boxseeker as OB

    d = np.load(os.path.join(GOLD, f"boxseeker_seed{seed}.npz"))
    sc = syn.make_seeker_scene(seed)
    assert ("aug" in sc["variant"]) == (seed == 3)
    want, cams = SP.ragged(d, "geom_out"), d["geom_cam"]
    pts = sc["points"][:, 1:4]
    boxes, labels, scores, _, cam_of = sc["dets"]
    k = n = 0
    for c in OB.IMAGE_ORDER:
        m = cam_of == c
        if not m.any():
            continue
        keep = OB.batched_nms_2d(boxes[m], scores[m], labels[m], PARAMS["nms_2d"])
        uvd, on = OB.project_to_camera(pts, sc["lidar_aug_matrix"][0], sc["lidar2image"][0, c].astype(np.float32))
        uvd = uvd[on]
        for box, score in zip(boxes[m][keep], scores[m][keep]):
            if score < PARAMS["score_thr"]:
                continue
            x1, y1, x2, y2 = box
            inb = (uvd[:, 1] < y2) & (uvd[:, 1] >= y1) & (uvd[:, 0] < x2) & (uvd[:, 0] >= x1)
            if not inb.any():
                continue
            fr, wc, _ = SP.restated_frustum(uvd[inb, 2], None, None, box, sc, c, PARAMS)
            assert want[k].shape == (1, 3) and want[k + 1].shape == (8, 3) and cams[k] == cams[k + 1] == c
            SP.check_frustum(wc, want[k][0])
            SP.check_frustum(fr, want[k + 1])
            k += 2
            n += 1
    # (the reference's third call per frustum back-projects its points, :812-815)
    assert n >= 10 and len(want) == 3 * n, "every frustum the reference built was compared"


def _camera_scene(n, seed):
    """points in front of camera 0 (plain cameras, identity lidar_aug_matrix), none within EDGE_PX of the box's or image's edges"""
    rng = np.random.default_rng(seed)
    sc = dict(syn.make_cameras(1))
    xyz = np.stack([rng.uniform(4.0, 45.0, n), rng.uniform(-25.0, 25.0, n), rng.uniform(-4.0, 6.0, n)], 1).astype(np.float32)
    box = np.array([200.0, 100.0, 1400.0, 800.0], np.float32)
    inside, graze = SP.selection64(SP.project64(xyz, sc, 0), box)
    xyz = xyz[~graze]
    return sc, xyz, box


def test_selection_check_catches_a_dropped_a_doubled_and_a_foreign_point():
    sc, xyz, box = _camera_scene(40_000, 1)
    u64, u32 = SP.project64(xyz, sc, 0), SP.project32(xyz, sc, 0)
    inside, graze = SP.selection64(u64, box)
    keep = np.ones(len(xyz), bool)
    keep[np.nonzero(inside)[0][10_000:]] = False          # exactly 10,000 points in the box, thousands around it
    u64, u32, inside = u64[keep], u32[keep], inside[keep]
    assert inside.sum() == 10_000 and (~inside).sum() > 5_000 and not graze.any()
    rng = np.random.default_rng(2)
    lst = u32[inside][rng.permutation(10_000)]            # (the order of the kernel's list is free)
    assert SP.check_selection(lst, u64, u32, box) == (10_000, 0)
    with pytest.raises(AssertionError, match="9999 points selected"):
        SP.check_selection(np.delete(lst, 1234, 0), u64, u32, box)
    doubled = lst.copy()
    doubled[77] = doubled[78]                             # the count is right, one point twice and another missing
    with pytest.raises(AssertionError, match="no point of the scene"):
        SP.check_selection(doubled, u64, u32, box)
    foreign = lst.copy()
    foreign[500, 2] = np.float32(foreign[500, 2] * (1 + 1e-5))   # a depth 80 ulp off
    with pytest.raises(AssertionError, match="no point of the scene"):
        SP.check_selection(foreign, u64, u32, box)
    outside = lst.copy()
    outside[9] = u32[np.nonzero(~inside)[0][0]]          # a point of the scene, but not of this box
    with pytest.raises(AssertionError, match="no point of the scene"):
        SP.check_selection(outside, u64, u32, box)
    # exact copies of rows (the tied depths of the large-frustum scene) are told apart by their number
    twice = np.concatenate([lst, u32[inside][:5]])
    with pytest.raises(AssertionError):
        SP.check_selection(twice, u64, u32, box)
    assert SP.check_selection(twice, np.concatenate([u64, u64[inside][:5]]), np.concatenate([u32, u32[inside][:5]]), box) == (10_005, 0)
    with pytest.raises(AssertionError):                  # (the wrong five rows twice)
        SP.check_selection(np.concatenate([lst, lst[:5]]), np.concatenate([u64, u64[inside][:5]]), np.concatenate([u32, u32[inside][:5]]), box)


def _depths(seed, m=10_000):
    rng = np.random.default_rng(seed)
    return rng.uniform(3.0, 45.0, m).astype(np.float32)


def _shifted(s, q):          # planted: rank lo (and with it hi) one too high
    m = s.shape[0]
    rank = np.float32(q) * np.float32(m - 1)
    lo, hi = int(np.floor(rank)) + 1, min(int(np.ceil(rank)) + 1, m - 1)
    a, b = s[lo], s[hi]
    w = np.float32(rank - np.float32(lo - 1))
    return np.float32(a + w * (b - a)) if w < 0.5 else np.float32(b - (b - a) * (np.float32(1) - w))


def _next_distinct(s, q):    # planted: the "(lo + 1)-th smallest" taken as the smallest key above a, also where a is duplicated
    m = s.shape[0]
    rank = np.float32(q) * np.float32(m - 1)
    lo, hi = int(np.floor(rank)), int(np.ceil(rank))
    a = s[lo]
    b = a if hi == lo else s[s > a].min()
    w = np.float32(rank - np.float32(lo))
    return np.float32(a + w * (b - a)) if w < 0.5 else np.float32(b - (b - a) * (np.float32(1) - w))


def test_quantile_restatement_matches_torch_and_the_oracle():
    import torch
    from oracle import boxseeker as OB

    for m in (1, 2, 3, 1000, 10_000):
        x = _depths(m, m)
        x[: m // 3] = x[m // 2]                           # a third of the list tied
        s = np.sort(x)
        for q in (0.0, 0.25, 0.336, 0.356, 0.46, 1.0):
            got = SP.quantile_sorted(s, q)
            assert got == OB.quantile(x, q)
            assert got == pytest.approx(float(torch.quantile(torch.from_numpy(x), q)), rel=1e-6)


def test_frustum_check_catches_a_shifted_rank_and_a_skipped_duplicate():
    sc = dict(syn.make_cameras(1))
    box = np.array([300.0, 200.0, 900.0, 700.0], np.float32)
    d = _depths(5)
    want, _, q = SP.restated_frustum(d, None, None, box, sc, 2, DEFAULT_Q)
    SP.check_frustum(SP.restated_frustum(d[::-1].copy(), None, None, box, sc, 2, DEFAULT_Q)[0], want)   # order is free
    got, _, q1 = SP.restated_frustum(d, None, None, box, sc, 2, DEFAULT_Q, quantile=_shifted)
    assert q1 != q
    with pytest.raises(AssertionError):
        SP.check_frustum(got, want)
    # without ties the second defect is none: the next distinct key IS the (lo + 1)-th smallest
    SP.check_frustum(SP.restated_frustum(d, None, None, box, sc, 2, DEFAULT_Q, quantile=_next_distinct)[0], want)
    # ties that straddle lo / hi of every rank: a run of equal depths from lo - 1 to lo + 2
    s = np.sort(d)
    for qv in (DEFAULT_Q["lq"], DEFAULT_Q["uq"], DEFAULT_Q["cq"]):
        lo = int(np.floor(np.float32(qv) * np.float32(len(s) - 1)))
        s[lo - 1: lo + 3] = s[lo]
        assert s[lo + 3] - s[lo] > 1e-3
    tied = s[np.random.default_rng(6).permutation(len(s))]
    want_t, _, qt = SP.restated_frustum(tied, None, None, box, sc, 2, DEFAULT_Q)
    assert qt[0] == s[int(np.floor(np.float32(DEFAULT_Q["lq"]) * np.float32(len(s) - 1)))], "a tied rank interpolates to the tie"
    got_t = SP.restated_frustum(tied, None, None, box, sc, 2, DEFAULT_Q, quantile=_next_distinct)[0]
    with pytest.raises(AssertionError):
        SP.check_frustum(got_t, want_t)
    # the clamp against the points' extent (clamp_bottom) damps a wrong far quantile only on the axes it binds
    lo3, hi3 = want.min(0) + 0.5, want.max(0) - 0.5
    clamped = SP.restated_frustum(d, lo3, hi3, box, sc, 2, dict(DEFAULT_Q, clamp_bottom=1))[0]
    assert (clamped.min(0) >= lo3 - 1e-6).all() and (clamped.max(0) <= hi3 + 1e-6).all()


def test_count_and_choice_checks_catch_one_count_and_one_choice():
    from oracle import boxseeker as OB

    rng = np.random.default_rng(9)
    prm = {"dns_w": 0.05, "iou_w": 0.95, "dst_w": 0.226}
    bb, bc = OB.base_proposals(dict(OB.DEFAULT_PARAMS, num_sizes=4))
    NC = 6 * bc.shape[1]
    valid = rng.integers(0, 3, NC).astype(np.int32)
    count = rng.integers(0, 9000, NC).astype(np.int32)
    iou = rng.uniform(0.3, 0.9, NC).astype(np.float32)
    want = count[valid == 2].copy()
    SP.check_counts(count, valid, want)
    off = count.copy()
    off[np.nonzero(valid == 2)[0][3]] += 1
    with pytest.raises(AssertionError):
        SP.check_counts(off, valid, want)
    sc = dict(syn.make_cameras(1))
    fr, wc, _ = SP.restated_frustum(_depths(3), None, None, np.array([300.0, 200.0, 900.0, 700.0], np.float32), sc, 0, DEFAULT_Q)
    s = SP.restated_scores(fr, wc, bc[0], OB.linspace_f32(0, 1, 6), valid, iou, count, prm)
    assert np.isnan(s[valid != 2]).all() and not np.isnan(s[valid == 2]).any()
    order = np.argsort(np.where(np.isnan(s), -np.inf, s))[::-1]
    assert s[order[0]] - s[order[1]] > 1e-4
    assert SP.check_choice(int(order[0]), s) is False
    with pytest.raises(AssertionError):
        SP.check_choice(int(order[1]), s)
    with pytest.raises(AssertionError):
        SP.check_choice(int(np.nonzero(valid != 2)[0][0]), s)
    # a count that is off moves the density term: the score of that candidate, and with a larger maximum every score
    s_off = SP.restated_scores(fr, wc, bc[0], OB.linspace_f32(0, 1, 6), valid, iou, off, prm)
    assert np.nanmax(np.abs(s_off - s)) > 0
    # near-tied top two: either passes, nothing else does
    t = s.copy()
    t[order[1]] = t[order[0]] - 5e-5
    assert SP.check_choice(int(order[1]), t) is True and SP.check_choice(int(order[0]), t) is True
    with pytest.raises(AssertionError):
        SP.check_choice(int(order[2]), t)
    assert SP.check_choice(-1, np.full(NC, np.nan)) is False
