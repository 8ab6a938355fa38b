"""Shared Box Seeker parity rule (tests/test_oracle_boxseeker.py on the CPU oracle, tests/test_gpu_boxseeker.py on the
HIP kernel) against the golden vectors the reference's own get_proposals produced
(tests/golden/make_boxseeker_golden.py).

For every frustum that yields a box the implementation under test reports which candidate it chose.  The rule:
  * that candidate is one of the candidates the reference scored, and its REFERENCE second-stage score
    (frustum_proposals_v1.py:997, recorded at the nms_normal_gpu call) lies within `tol` of the reference's maximum,
    where tol = 1e-4 (2D-IoU rounding, rtol 1e-4 on values <= 1) + 2 * (largest point-count difference between the
    implementation and the reference inside this frustum) / (reference max count): zero count differences leave only
    the float noise, so a wrong choice cannot hide behind the tolerance;
  * the returned box equals the reference's own box of THAT candidate (the row it handed to points_in_boxes_gpu)
    in all 7 components to BOX_ATOL;
  * when the reference's top score is unique beyond tol the box therefore equals the reference's output box.
What the count allowance is (round 6): NOT a tolerance between two point-in-box implementations — on the GPU box every
per-candidate count of the kernel is held to the reference's own points_in_boxes kernel with array_equal
(tests/test_gpu_boxseeker.py _counts_equal_the_reference_kernel, oracle/_ref/libref_pib_gpu.so) — but between the kernel's run and
the FIXTURE's run of the reference, whose candidate boxes equal the kernel's to 1e-4, not bit for bit (torch f32 vs the kernel's
f32 arithmetic), so a point within that distance of a face may fall on the other side.
Exact ties (yaw 0 vs pi footprints, the six identical depth samples of a collapsed frustum) are the only freedom left:
the reference's own unstable sort (iou3d_nms_utils.py:146) decides them.
"""
import numpy as np

BOX_ATOL = 1e-4      # north_star: box regressions within 1e-4 (f32); coordinates reach 54 m (ulp 3.8e-6)


def ragged(d, key):
    off = d[key + "_off"]
    return [d[key][off[i]:off[i + 1]] for i in range(len(off) - 1)]


def check_choices(d, out_boxes, chosen, extra_tol=0.0):
    """d: golden npz; out_boxes (K,7); chosen: per output box (scored candidate ids ascending, chosen candidate id,
    point counts of the scored candidates).  extra_tol: added to the score tolerance when the distance term is on
    (dst_w > 0): the reference ranks the candidates by torch.cdist, whose matmul formulation (|a|^2 + |b|^2 - 2ab in f32,
    used above 25 rows) carries ~1e-3 of relative error on sub-metre distances — not something to reproduce."""
    ws = ragged(d, "nms3d_scores") if "nms3d_scores" in d.files else []
    assert len(ws) == out_boxes.shape[0] == len(chosen) == d["out_boxes"].shape[0]
    offs = np.cumsum([0] + [len(w) for w in ws])
    n_unique = n_tied_ref = n_loose = 0
    for k, (cand_ids, best, counts) in enumerate(chosen):
        w = ws[k][:, 0]
        seg = slice(offs[k], offs[k + 1])
        ref_boxes, ref_counts = d["pib_box"][seg], d["pib_count"][seg]
        assert len(cand_ids) == len(w), f"frustum {k}: scored candidate sets differ"
        pos = list(cand_ids).index(best)
        dcount = np.abs(np.asarray(counts, np.int64) - ref_counts).max()
        tol = 1e-4 + extra_tol + 2.0 * dcount / max(int(ref_counts.max()), 1)
        assert w[pos] >= w.max() - tol, f"frustum {k}: chose a candidate {w.max() - w[pos]:.3e} below the reference's best (tol {tol:.1e})"
        np.testing.assert_allclose(out_boxes[k], ref_boxes[pos], rtol=0, atol=BOX_ATOL, err_msg=f"frustum {k}")
        top = np.sort(w)[::-1]
        if len(top) == 1 or top[0] - top[1] > tol:
            n_unique += 1
            np.testing.assert_allclose(out_boxes[k], d["out_boxes"][k], rtol=0, atol=BOX_ATOL, err_msg=f"frustum {k}")
        elif top[0] - top[1] <= 1e-4 + extra_tol:
            n_tied_ref += 1          # a tie in the FIXTURE (yaw 0 vs pi, collapsed frustum): the reference's own sort decides it
        else:
            n_loose += 1             # decided only because a point count differed (widened tolerance)
    # every frustum the fixture itself decides beyond float noise must have been checked against the reference's OUTPUT box
    assert n_unique + n_tied_ref + n_loose == len(chosen)
    return n_unique, n_tied_ref, n_loose


def check_choices_oracle(trace, out_boxes, chosen):
    """The same rule against a trace of oracle/boxseeker.get_proposals (fresh scenes, parameter variants): the chosen
    candidate's ORACLE score within tol of the oracle's best, and the box equal to the oracle's box of that candidate."""
    scored = [t for t in trace if "scores" in t]
    assert len(scored) == out_boxes.shape[0] == len(chosen)
    for k, (t, (cand_ids, best, counts)) in enumerate(zip(scored, chosen)):
        assert list(cand_ids) == list(t["idx_final"]), f"frustum {k}: scored candidate sets differ"
        pos = list(cand_ids).index(best)
        dcount = np.abs(np.asarray(counts, np.int64) - t["counts"].astype(np.int64)).max()
        assert dcount <= 2
        tol = 1e-4 + 2.0 * dcount / max(int(t["counts"].max()), 1)
        w = t["scores"]
        assert w[pos] >= w.max() - tol, f"frustum {k}: {w.max() - w[pos]:.3e} below the oracle's best (tol {tol:.1e})"
        np.testing.assert_allclose(out_boxes[k], t["cand_boxes"][best], rtol=0, atol=BOX_ATOL, err_msg=f"frustum {k}")


# ------------------------------------------------------------------------------------------------------------------------
# Plain restatement of the kernel's per-frustum front end (csrc/boxseeker.hip stages A-D) and of its counting and choice (G, H),
# for frustums too large for the full oracle (tests/test_gpu_boxseeker_batches.py; held to the reference's recording and to
# planted defects by tests/test_seeker_frontend_ref.py).  Every check works from the kernel's own debug lists.
SEEKER_LAT_MAX_FRUSTUMS = 512    # fnp_boxseeker (csrc/boxseeker.hip): `lat = num_frustums <= 512` — the two move together
EDGE_PX = 1e-3                   # a point this close to an edge of its box / the image may fall on either side in f32
IMAGE_H, IMAGE_W = 900, 1600
F32 = np.float32


def project64(xyz, sc, cam):
    """project_to_camera (:1431-1475) in float64 from the scene's own f32 matrices -> (N, 3) [u, v, depth]."""
    aug = sc["lidar_aug_matrix"][0].astype(np.float64)
    L = sc["lidar2image"][0, cam].astype(np.float64)
    p = (np.asarray(xyz, np.float64) - aug[:3, 3]) @ np.linalg.inv(aug[:3, :3]).T
    q = p @ L[:3, :3].T + L[:3, 3]
    d = np.clip(q[:, 2], 1e-5, 1e5)
    uvd = np.stack([q[:, 0] / d, q[:, 1] / d, d], 1)
    if "img_aug_matrix" in sc:
        A = sc["img_aug_matrix"][0, cam].astype(np.float64)
        uvd = uvd @ A[:3, :3].T + A[:3, 3]
    return uvd


def project32(xyz, sc, cam):
    """The kernel's own f32 expression order (project() of csrc/boxseeker.hip; identity lidar_aug_matrix, no img_aug_matrix):
    IEEE multiplies, adds and one division per coordinate, so numpy's f32 gives the same bits."""
    assert np.array_equal(sc["lidar_aug_matrix"][0], np.eye(4, dtype=F32)) and "img_aug_matrix" not in sc
    L = sc["lidar2image"][0, cam].astype(F32)
    x, y, z = (np.ascontiguousarray(xyz[:, i], F32) for i in range(3))
    q = [(L[r, 0] * x + L[r, 1] * y) + L[r, 2] * z + L[r, 3] for r in range(3)]
    d = np.minimum(np.maximum(q[2], F32(1e-5)), F32(1e5))
    return np.stack([q[0] / d, q[1] / d, d], 1).astype(F32)


def selection64(uvd, box):
    """uvd (N, 3) float64, box [x1, y1, x2, y2] -> (inside (N,), grazing (N,)): the reference's test (:606-613: on the image and
    in the box, lower edges included) and the points within EDGE_PX of the boundary of that region."""
    x1, y1, x2, y2 = (float(v) for v in box)
    lo_u, hi_u, lo_v, hi_v = max(x1, 0.0), min(x2, float(IMAGE_W)), max(y1, 0.0), min(y2, float(IMAGE_H))
    u, v = uvd[:, 0], uvd[:, 1]
    inside = (u >= lo_u) & (u < hi_u) & (v >= lo_v) & (v < hi_v)
    margin = np.minimum(np.minimum(u - lo_u, hi_u - u), np.minimum(v - lo_v, hi_v - v))
    return inside, np.abs(margin) <= EDGE_PX


def _multiset_excess(a, b):
    """rows (as bits) of a that b does not hold as often, and the other way round: (rows of a (k, 3), indices into b)"""
    ua = np.ascontiguousarray(a, F32).view(np.uint32).reshape(-1, 3)
    ub = np.ascontiguousarray(b, F32).view(np.uint32).reshape(-1, 3)
    uniq, inv = np.unique(np.concatenate([ua, ub]), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    ca = np.bincount(inv[:len(ua)], minlength=len(uniq))
    cb = np.bincount(inv[len(ua):], minlength=len(uniq))
    more_a = np.repeat(np.arange(len(uniq)), np.maximum(ca - cb, 0))
    left_b = []
    inv_b = inv[len(ua):]
    for k in np.nonzero(cb > ca)[0]:
        left_b.extend(np.nonzero(inv_b == k)[0][: cb[k] - ca[k]].tolist())
    return uniq[more_a].view(F32).reshape(-1, 3), np.asarray(left_b, np.int64)


def check_selection(list_uvd, scene_uvd64, scene_uvd32, box):
    """Stage A of one frustum.  list_uvd: the kernel's own (npts, 3) list; scene_uvd64 / scene_uvd32: the scene's points in this
    frustum's camera (project64 / project32).  Rules: |npts - count64| <= g with g the number of grazing points, and the list is
    a sub-multiset of the scene's rows that are inside or grazing which misses none of the rows inside beyond EDGE_PX.  A row
    that does not match bit for bit may match a still unmatched row within 4 ulp per component (nothing else of f32 arithmetic
    is free).  Returns (count64, g)."""
    inside, graze = selection64(scene_uvd64, box)
    count64, g = int(inside.sum()), int(graze.sum())
    npts = int(list_uvd.shape[0])
    assert abs(npts - count64) <= g, f"{npts} points selected, {count64} in float64, {g} within {EDGE_PX} px of an edge"
    pool = np.nonzero(inside | graze)[0]
    more, left = _multiset_excess(list_uvd, scene_uvd32[pool])
    left = list(left)
    for row in more:                       # (none when the arithmetic agrees bit for bit)
        assert left, f"the kernel's list holds {row}, which is no point of the scene inside this box"
        c = scene_uvd32[pool[left]]
        err = (np.abs(c.astype(np.float64) - row.astype(np.float64)) / np.spacing(np.abs(c)).astype(np.float64)).max(1)
        j = int(np.argmin(err))
        assert err[j] <= 4.0, f"the kernel's list holds {row}, which is no point of the scene inside this box (nearest {c[j]})"
        left.pop(j)
    assert graze[pool[left]].all(), f"{(~graze[pool[left]]).sum()} points inside the box (beyond {EDGE_PX} px) are not in the kernel's list"
    return count64, g


def quantile_sorted(s, q):
    """torch.quantile(x, q) on the ascending f32 list s, as quantile() of csrc/boxseeker.hip evaluates it: rank = q (m - 1) in
    f32, a = s[floor], b = s[ceil] (b is a again when a is duplicated past floor), torch.lerp's two-sided f32 form."""
    m = s.shape[0]
    rank = F32(q) * F32(m - 1)
    lo, hi = int(np.floor(rank)), int(np.ceil(rank))
    a, b = F32(s[lo]), F32(s[hi])
    w = F32(rank - F32(lo))
    return F32(a + w * (b - a)) if w < F32(0.5) else F32(b - (b - a) * (F32(1) - w))


def restated_frustum(depths, xyz_min, xyz_max, box, sc, cam, prm, quantile=quantile_sorted):
    """Stages B-D for one frustum from the kernel's own depth list (m,) and the exact per-axis min / max of its lidar-frame points:
    -> (the frustum's 8 corners in lidar as the kernel leaves them (clamp_bottom applied when prm sets it), the weighted centre
    (3,), the three quantiles).  Geometry through the oracle's get_cam_frustum and get_geometry_at_image_coords."""
    from oracle import boxseeker as OB
    s = np.sort(np.asarray(depths, np.float64)).astype(F32)
    qlo, qhi, qc = (quantile(s, prm[k]) for k in ("lq", "uq", "cq"))
    x1, y1, x2, y2 = (F32(v) for v in box)
    fmax, fmin = min(qhi, F32(prm.get("max_dist", 50.0))), max(qlo, F32(2.0))          # :647-648
    c2l, K, aug = sc["camera2lidar"][0, cam], sc["camera_intrinsics"][0, cam], sc["lidar_aug_matrix"][0].astype(F32)
    ia = sc["img_aug_matrix"][0, cam].astype(F32) if "img_aug_matrix" in sc else None
    fr = OB.geometry_at_image_coords(OB.cam_frustum(np.array([x1, y1, fmin, x2, y2, fmax], F32)), c2l, K, aug, ia)
    wc = OB.geometry_at_image_coords(np.array([[(x1 + x2) / F32(2), (y1 + y2) / F32(2), qc]], F32), c2l, K, aug, ia)[0]
    if prm.get("clamp_bottom", 0) > 0:                                                # :817-826
        f1 = np.maximum(np.asarray(xyz_min, F32), fr.min(0))
        f2 = np.minimum(np.asarray(xyz_max, F32), fr.max(0))
        fr = np.minimum(np.maximum(fr, f1[None]), f2[None])
    return fr.astype(F32), wc.astype(F32), (qlo, qhi, qc)


def check_frustum(got, want):
    np.testing.assert_allclose(got, want, rtol=0, atol=BOX_ATOL)


def check_counts(count, valid, want):
    """count, valid: the kernel's (NC,) rows of one frustum; want: the point-in-box operator's counts of the scored candidates."""
    ids = np.nonzero(valid == 2)[0]
    assert np.array_equal(count[ids], np.asarray(want)), f"candidates {ids[count[ids] != np.asarray(want)]}: {count[ids]} != {want}"


def restated_scores(fr, wc, base_corners, mags, valid, iou, count, prm):
    """Second-stage scores (:994-997, MULT off) of one frustum in float64 from the kernel's own corners fr (8, 3), weighted centre
    wc, 2D IoUs and counts; base_corners (R, 8, 3) of the frustum's label.  NaN where the candidate was not scored."""
    fr, wc = np.asarray(fr, np.float64), np.asarray(wc, np.float64)
    bev = np.stack([(fr[2 * i] + fr[2 * i + 1]) / 2 for i in range(4)])               # :828
    close, far = (bev[0] + bev[1]) / 2, (bev[2] + bev[3]) / 2
    pts = close[None] + (far - close)[None] * np.asarray(mags, np.float64)[:, None]   # :845
    corners = (np.asarray(base_corners, np.float64)[None] + pts[:, None, None, :]).reshape(-1, 8, 3)
    nrm = np.sqrt((corners * corners).sum(2))                                         # :863 softmin over the 8 corners
    e = np.exp(-(nrm - nrm.min(1, keepdims=True)))
    wfc = ((e / e.sum(1, keepdims=True))[..., None] * corners).sum(1)
    dd = np.sqrt(((wfc - wc[None]) ** 2).sum(1))                                      # :886-893, over the distance-valid set
    out = np.full(valid.shape, np.nan)
    sc = valid == 2
    if not sc.any():
        return out
    dv = valid >= 1
    dr = 1.0 - (dd - dd[dv].min()) / (dd[dv].max() - dd[dv].min() + 1e-8)
    soft = count.astype(np.float64) / (count[sc].max() + 1e-8)
    s = soft * prm["dns_w"] + iou.astype(np.float64) * prm["iou_w"] + dr * prm["dst_w"]
    out[sc] = s[sc]
    return out


def check_choice(best, scores):
    """best: the kernel's out_best of one frustum; scores: restated_scores.  The argmax; where the top two are closer than 1e-4
    any candidate within 1e-4 of the top passes.  Returns whether the frustum was that close."""
    ids = np.nonzero(~np.isnan(scores))[0]
    if len(ids) == 0:
        assert best == -1
        return False
    top = np.sort(scores[ids])[::-1]
    near = len(top) > 1 and top[0] - top[1] < 1e-4
    assert best in ids, f"chose {best}, which was not scored"
    if near:
        assert scores[best] > top[0] - 1e-4, f"chose {best}, {top[0] - scores[best]:.3e} below the best"
    else:
        assert best == ids[int(np.argmax(scores[ids]))], f"chose {best}, {top[0] - scores[best]:.3e} below the best"
    return bool(near)


# The subset's seed is part of the scene: it is chosen (with oracle/boxseeker.py on the CPU, seeds 0-55) so that the scene meets
# the conditions the large-frustum test puts on its INPUT — no frustum with more than three grazing points, every whole-image
# frustum above 10,000 points, and at most 3 of its 30 frustums with their two best candidates within 1e-4 under each of the
# four parameter sets.  The last one is narrow by nature: yaw 0 and yaw pi are the same footprint, so a frustum whose best yaw
# is 0 ties exactly, which 2-7 frustums of a scene of this family do.
LARGE_SCENE_SUBSET_SEED = 54


def large_tied_scene(subset_seed=LARGE_SCENE_SUBSET_SEED, n_points=125_000, n_copies=5_000):
    """One scene with frustums of tens of thousands of points and many bitwise-equal depths: a seeded subset of the ten-sweep
    scene 0 (synthetic.make_sweeps_batch, 306,508 points) plus exact copies of n_copies of its own rows, the cameras and
    detections of make_seeker_scene(0), and per camera one whole-image and one half-image detection.  The two of a camera carry
    different labels (the 2D NMS is per label; there are ten classes, so the twelve share labels across cameras only)."""
    from findnpropagate_amd import synthetic as syn
    sc = syn.make_seeker_scene(0)
    allp, _ = syn.make_sweeps_batch([0])
    rng = np.random.default_rng(subset_seed)
    sub = allp[np.sort(rng.choice(allp.shape[0], n_points, replace=False))]
    pts = np.concatenate([sub, sub[rng.choice(n_points, n_copies, replace=False)]])
    sc["points"] = np.concatenate([np.zeros((pts.shape[0], 1), np.float32), pts], axis=1)
    b, l, s, bi, ci = sc["dets"]
    eb = np.array([[0, 0, IMAGE_W, IMAGE_H], [0, 0, IMAGE_W // 2, IMAGE_H]] * 6, np.float32)
    el = np.array([(2 * c + k) % 10 + 1 for c in range(6) for k in range(2)], np.int64)
    sc["dets"] = (np.concatenate([b, eb]), np.concatenate([l, el]), np.concatenate([s, np.full(12, 0.9, np.float32)]),
                  np.concatenate([bi, np.zeros(12, np.int64)]), np.concatenate([ci, np.repeat(np.arange(6), 2)]))
    return sc
