"""The Box Seeker kernel (csrc/boxseeker.hip) on both sides of its dispatch bound, and on frustums and scene sizes the fixture
scenes do not reach.

fnp_boxseeker picks boxseeker_kernel<OPT, LAT>: LAT (the latency form: workgroup-parallel bin search in the radix select, four
points per thread per trip of the point scan) up to SEEKER_LAT_MAX_FRUSTUMS frustums per launch, the throughput form (thread 0
walks the histogram bins, one point per thread per trip) above.  The fixture scenes hold 10-23 frustums, so every other value
test launches the latency form; the throughput form is what a batched extraction and the benchmark's Box Seeker figure run.
  1  shipped path, 32 and 48 fixture scenes per launch, every scene copy against the reference's recorded run and against
     the same scene launched alone;
  2  the options no shipped configuration sets (and seeds 16 / 17), enough copies of one scene to cross the bound;
  3  frustums of more than 10,000 points with thousands of bitwise-equal depths, against the plain restatement of
     tests/seeker_parity.py (held to the reference by tests/test_seeker_frontend_ref.py);
  4  scene sizes around the trips of the point scan (256 and 1024 rows) and empty scenes in a batch;
  5  extract_pseudo_labels with 48 scenes per step against 2 per step.
Two forms differ only in the order of a frustum's point list, and everything behind the list is an integer atomic, a min / max
or an order statistic: a scene's outputs are required to be the same BITS in any batch, on either side of the bound.
Every launch is made twice (same bits) and once more without the debug tensors (same bits again); outputs are torch.empty, and
every element of them is compared with something, so an element the kernel left unwritten shows.
Each case prints one line (frustums of the launch, form, largest frustum) — DESIGN.md "Box Seeker at batch size" keeps a copy."""
import math
import os
import tempfile

import numpy as np
import pytest
import torch

import seeker_parity as SP
from findnpropagate_amd import synthetic as syn
from seeker_parity import BOX_ATOL, SEEKER_LAT_MAX_FRUSTUMS, check_choices, ragged
from test_gpu_boxseeker import GOLD, PARAMS, _batch, _counts_equal_the_reference_kernel, _head
from test_gpu_extract import nccl_world1  # noqa: F401  (the world-size-1 RCCL group of the extraction tests, as a fixture of this module)

pytestmark = pytest.mark.gpu
OUT_KEYS = ("out_count", "out_valid", "out_box", "out_score", "out_best")
DBG_KEYS = ("npts", "frust", "cand", "iou", "count", "valid")
DEFAULT_QUANTILES = {"lq": 0.336, "uq": 0.356, "iou_w": 0.95, "dst_w": 0.226, "dns_w": 0.05, "cq": 0.46, "num_sizes": 4}   # (:144-147)


def _same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.float32:      # (a NaN score — search_depth on a collapsed frustum — is a value like any other here)
        a, b = a.view(torch.int32), b.view(torch.int32)
    return torch.equal(a, b)


def _is_option(pv):
    p, c = pv
    return bool(p.get("topk", 1) > 1 or p.get("search_depth") or p.get("occl_w", 0) > 0 or p.get("rand_center") or c.get("OCCL_MULT")
                or c.get("MULTICAM_IOU"))


def _launch(head, bd, form, noise=None):
    """One launch of the batch, checked as every launch of this module is: the frustum count lies on the stated side of the
    dispatch bound, a second launch and a launch without debug tensors give the same bits.  -> (result, F, TK)"""
    with torch.no_grad():
        r = head.launch(bd, debug=True, noise=noise)
        again = head.launch(bd, debug=True, noise=noise)
        plain = head.launch(bd, debug=False, noise=noise)
    F = r["out_count"].shape[0]
    assert form in ("latency", "throughput") and (F <= SEEKER_LAT_MAX_FRUSTUMS) == (form == "latency"), (F, form)
    TK = r["out_box"].shape[0] // F
    assert r["out_box"].shape == (F * TK, 7) and r["out_valid"].shape == r["out_score"].shape == r["out_best"].shape == (F * TK,)
    assert r["frustums"].shape == (F * TK, 8) and TK == int(head.topk)
    for k in OUT_KEYS:
        assert _same_bits(r[k], again[k]) and _same_bits(r[k], plain[k]), k
    for k in DBG_KEYS:
        assert r["dbg"][k].shape[0] == F and _same_bits(r["dbg"][k], again["dbg"][k]), k
    return r, F, TK


def _scene_ranges(r, TK, n_scenes):
    """per scene of the batch the range [lo, hi) of its frustums (they are enumerated scene by scene)"""
    ids = r["frustums"][::TK, 0].numpy().astype(np.int64)
    assert (np.diff(ids) >= 0).all()
    return [(int(np.searchsorted(ids, b, "left")), int(np.searchsorted(ids, b, "right"))) for b in range(n_scenes)]


def _cut(r, lo, hi, TK):
    """the rows of frustums lo .. hi - 1 of every output and debug tensor (device views)"""
    s = {"out_count": r["out_count"][lo:hi]}
    for k in OUT_KEYS[1:]:
        s[k] = r[k][lo * TK: hi * TK]
    for k in DBG_KEYS:
        s[k] = r["dbg"][k][lo:hi]
    s["rows"] = r["frustums"][lo * TK: hi * TK, 1:]       # (camera, box, label, score: all but the scene number)
    return s


def _assert_same_scene(a, b, what):
    for k in OUT_KEYS + DBG_KEYS:
        assert _same_bits(a[k], b[k]), f"{what}: {k} differs"
    assert torch.equal(a["rows"], b["rows"]), what


def _host(s):
    return {k: v.cpu().numpy() for k, v in s.items()}


def _record(part, F, form, path, npts):
    largest = f", largest frustum {int(npts.max())} points" if npts is not None and len(npts) else ""
    print(f"\n[boxseeker batches] part {part}: {F} frustums, {form} form, {path} path{largest}", end="")


def _golden_rules(d, sc, pv, S):
    """The checks of test_gpu_boxseeker.test_matches_reference_golden on one scene copy's rows S (host arrays, topk 1)."""
    has = S["out_valid"].astype(bool)
    boxes, labels, scores = S["out_box"][has], S["rows"][has, 5].astype(np.int64), S["rows"][has, 6]
    assert boxes.shape == d["out_boxes"].shape
    assert labels.tolist() == d["out_labels"].tolist(), "same frustums yield a box, same order"
    np.testing.assert_allclose(scores, d["out_scores"], rtol=0, atol=1e-7)
    if boxes.shape[0] == 0:
        return
    valid, count = S["valid"], S["count"]
    scored = valid == 2
    counts, want = count[scored], d["pib_count"]
    assert counts.shape == want.shape, "same candidates survive max_dist and min_cam_iou"
    assert (counts != want).mean() < 0.01 and np.abs(counts - want).max() <= 2
    np.testing.assert_allclose(S["cand"][scored], d["pib_box"], rtol=0, atol=BOX_ATOL)
    want_iou = ragged(d, "iou_out")
    k = 0
    for f in range(valid.shape[0]):
        if S["npts"][f] == 0 or not (valid[f] >= 1).any():
            continue
        np.testing.assert_allclose(S["iou"][f][valid[f] >= 1], want_iou[k][:, 0], rtol=1e-4, atol=2e-5)
        k += 1
    assert k == len(d["iou_out_off"]) - 1
    chosen = []
    for f in range(valid.shape[0]):
        if has[f]:
            ids = np.nonzero(valid[f] == 2)[0]
            chosen.append((ids, int(S["out_best"][f]), count[f][ids]))
    n_unique, n_tied_ref, n_loose = check_choices(d, boxes, chosen, extra_tol=2e-3 * float(pv[0].get("dst_w", 0.0)))
    assert n_unique == boxes.shape[0] - n_tied_ref - n_loose and n_loose <= max(1, boxes.shape[0] // 10)
    if "lone_point" in sc["variant"]:
        assert ((S["npts"] == 1) & has).any(), "the single-return frustum yields a box"


def _option_rules(d, pv, tk, S):
    """The checks of test_gpu_boxseeker.test_option_variants_match_reference_golden on one scene copy's rows S (host arrays)."""
    from test_oracle_boxseeker import boxes_equal_mod_half_turn

    has = S["out_valid"].astype(bool)                      # (row form: tk rows per frustum)
    boxes, labels, scores = S["out_box"][has], S["rows"][has, 5].astype(np.int64), S["rows"][has, 6]
    assert boxes.shape == d["out_boxes"].shape and labels.tolist() == d["out_labels"].tolist()
    np.testing.assert_allclose(scores, d["out_scores"], rtol=0, atol=1e-7)
    same = boxes_equal_mod_half_turn(boxes, d["out_boxes"])
    assert same.mean() >= 0.9, f"{(~same).sum()} of {len(same)} boxes differ from the reference's beyond a half-turn tie"
    valid, count, cand = S["valid"], S["count"], S["cand"]
    occl = bool(pv[0].get("occl_w", 0) or pv[1].get("OCCL_MULT", False))
    calls = 1 + int(pv[0].get("occl_w", 0) > 0) + int(bool(pv[1].get("OCCL_MULT", False)))
    ws, sel = ragged(d, "nms3d_scores"), ragged(d, "nms3d_selected")
    n_out, out_score = S["out_count"], S["out_score"].reshape(-1, tk)
    pos = k = 0
    for f in range(valid.shape[0]):
        ids = np.nonzero(valid[f] == 2)[0]
        if len(ids) == 0:
            assert n_out[f] == 0
            continue
        np.testing.assert_allclose(cand[f][ids], d["pib_box"][pos: pos + len(ids)], rtol=0, atol=1e-4)
        ref_counts = d["pib_count"][pos: pos + len(ids)]
        assert np.abs(count[f][ids] - ref_counts).max() <= 2
        pos += calls * len(ids)
        assert n_out[f] == min(tk, len(sel[k]))
        ref_sel = ws[k][:, 0][sel[k][:, 0][: n_out[f]]]
        np.testing.assert_allclose(out_score[f][: n_out[f]], ref_sel, rtol=2e-2 if occl else 0, atol=1e-4 + 2.0 / max(float(ref_counts.max()), 1.0))
        k += 1
    assert pos == d["pib_box"].shape[0] and k == len(ws)


# ---- 1: shipped path, fixture scenes 0-15 in cycles ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shipped(cuda):
    """the 16 default-parameter fixture scenes, their recordings, and each launched alone (the latency form the rest of the suite
    holds to the reference): made once, left unchanged"""
    scenes = [syn.make_seeker_scene(s) for s in range(16)]
    gold = [np.load(os.path.join(GOLD, f"boxseeker_seed{s}.npz")) for s in range(16)]
    alone = []
    for sc in scenes:
        bd, dets = _batch([sc], cuda)
        head = _head(lambda _, dets=dets: dets)
        if head.enumerate_frustums(bd).shape[0] == 0:      # no_dets / low_scores: nothing to launch
            alone.append(None)
            continue
        r, F, TK = _launch(head, bd, "latency")
        alone.append(_cut(r, 0, F, TK))
    return scenes, gold, alone


@pytest.mark.parametrize("cycles, form", [(2, "latency"), (3, "throughput")])
def test_fixture_scenes_in_cycles_match_the_recording_and_the_scene_alone(cuda, shipped, cycles, form):
    scenes, gold, alone = shipped
    bd, dets = _batch(scenes * cycles, cuda)
    r, F, TK = _launch(_head(lambda _: dets), bd, form)
    rng_ = _scene_ranges(r, TK, 16 * cycles)
    assert sum(hi - lo for lo, hi in rng_) == F and TK == 1
    _record(1, F, form, "shipped", r["dbg"]["npts"].cpu().numpy())
    for b, (lo, hi) in enumerate(rng_):
        seed = b % 16
        S = _cut(r, lo, hi, TK)
        if alone[seed] is None:
            assert hi == lo and gold[seed]["out_boxes"].shape[0] == 0
            continue
        _assert_same_scene(S, alone[seed], f"scene {b} (seed {seed}) in the batch of {16 * cycles} vs alone")
        _golden_rules(gold[seed], scenes[seed], ({}, {}), _host(S))
    if form == "throughput":    # one copy of one seed against the reference's own point-in-box kernel (one launch per candidate)
        lo, hi = rng_[32]
        dbg = {k: r["dbg"][k][lo:hi] for k in ("valid", "count", "npts", "cand")}
        dbg["points_xyz"] = r["dbg"]["points_xyz"][lo:hi]
        _counts_equal_the_reference_kernel(dbg)


# ---- 2: option path (and seeds 16 / 17), copies of one scene past the bound ---------------------------------------------------
@pytest.mark.parametrize("seed", [16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 27])
def test_copies_of_one_scene_past_the_bound_match_the_recording_and_the_scene_alone(cuda, seed):
    from test_oracle_boxseeker import option_scene

    pv = syn.SEEKER_PARAM_VARIANTS[seed]
    if seed in (16, 17):
        d, sc, noise = np.load(os.path.join(GOLD, f"boxseeker_seed{seed}.npz")), syn.make_seeker_scene(seed), None
    else:
        d, sc, _, noise = option_scene(seed)
    tk = int(pv[0].get("topk", 1))
    now = {}
    head = _head(lambda _: now["dets"], dict(PARAMS, **pv[0]), pv[1])
    bd1, now["dets"] = _batch([sc], cuda)
    noise1 = None
    if noise is not None:     # the i-th recorded draw belongs to the i-th frustum that holds points (test_gpu_boxseeker.py)
        F1 = head.enumerate_frustums(bd1).shape[0]
        with torch.no_grad():
            r0 = head.launch(bd1, debug=True, noise=torch.zeros((F1, head.num_mags, 3), device=cuda))
        has_pts = np.nonzero(r0["dbg"]["npts"].cpu().numpy() > 0)[0]
        assert len(has_pts) == len(noise)
        noise1 = torch.zeros((F1, head.num_mags, 3))
        for f, draw in zip(has_pts, noise):
            noise1[f] = torch.from_numpy(draw)
        noise1 = noise1.to(cuda)
    r1, F1, TK = _launch(head, bd1, "latency", noise=noise1)
    one = _cut(r1, 0, F1, TK)
    n = math.ceil((SEEKER_LAT_MAX_FRUSTUMS + 1) / F1)
    bd, now["dets"] = _batch([sc] * n, cuda)
    r, F, TK = _launch(head, bd, "throughput", noise=None if noise1 is None else noise1.repeat(n, 1, 1))   # (the draws, per copy)
    assert F == n * F1 and TK == tk
    _record(2, F, "throughput", f"{'option' if _is_option(pv) else 'shipped'} (seed {seed}, {n} copies)", r["dbg"]["npts"].cpu().numpy())
    rules = (lambda S: _golden_rules(d, sc, pv, S)) if seed in (16, 17) else (lambda S: _option_rules(d, pv, tk, S))
    rules(_host(one))
    for b, (lo, hi) in enumerate(_scene_ranges(r, TK, n)):
        assert hi - lo == F1
        S = _cut(r, lo, hi, TK)
        _assert_same_scene(S, one, f"copy {b} of {n} vs the scene alone")     # (and with it vs copy 0)
        rules(_host(S))


# ---- 3: large frustums with tied depths ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large(cuda):
    """the scene, its points in every camera (float64 and in the kernel's f32 order), made once"""
    sc = SP.large_tied_scene()
    xyz = sc["points"][:, 1:4]
    _, inv, cnt = np.unique(np.ascontiguousarray(xyz[:, :3]).view(np.uint32).reshape(-1, 3), axis=0, return_inverse=True, return_counts=True)
    assert (cnt > 1).sum() >= 4_000, "thousands of bitwise-equal rows"
    u64 = [SP.project64(xyz, sc, c) for c in range(6)]
    u32 = [SP.project32(xyz, sc, c) for c in range(6)]
    return sc, u64, u32, {}


def _large_launches(cuda, large, prm_extra):
    """the scene alone and as copies past the bound under PARAMS + prm_extra (cached per parameter set)"""
    sc, _, _, cache = large
    key = tuple(sorted(prm_extra.items()))
    if key not in cache:
        prm = dict(PARAMS, **prm_extra)
        now = {}
        head = _head(lambda _: now["dets"], prm)
        bd1, now["dets"] = _batch([sc], cuda)
        r1, F1, _ = _launch(head, bd1, "latency")
        n = math.ceil((SEEKER_LAT_MAX_FRUSTUMS + 1) / F1)
        bd, now["dets"] = _batch([sc] * n, cuda)
        r, F, _ = _launch(head, bd, "throughput")
        assert F == n * F1 and F - F1 <= SEEKER_LAT_MAX_FRUSTUMS, "just above the bound (the scratch grows with F x points)"
        cache.clear()           # (one parameter set's launches at a time: the throughput launch's scratch is 1.7 GB)
        cache[key] = (head, prm, r1, F1, r, F, n)
    return cache[key]


def _selection_of(r, lo, hi, large):
    """check_selection on frustums lo .. hi - 1 of launch r -> (largest frustum, largest g, whole-image counts)"""
    sc, u64, u32, _ = large
    npts = r["dbg"]["npts"].cpu().numpy()
    rows = r["frustums"].numpy()
    g_max, whole = 0, []
    for f in range(lo, hi):
        cam, box = int(rows[f, 1]), rows[f, 2:6]
        lst = r["dbg"]["points_uvd"][f, : int(npts[f])].cpu().numpy()
        count64, g = SP.check_selection(lst, u64[cam], u32[cam], box)
        assert g <= 3, "the scene is built so that no frustum has more than three grazing points (large_tied_scene)"
        g_max = max(g_max, g)
        if tuple(box) == (0.0, 0.0, float(SP.IMAGE_W), float(SP.IMAGE_H)):
            whole.append(int(npts[f]))
    return int(npts[lo:hi].max()), g_max, whole


@pytest.mark.parametrize("form", ["latency", "throughput"])
def test_large_frustums_select_the_points_of_the_box(cuda, large, form):
    head, prm, r1, F1, r, F, n = _large_launches(cuda, large, {})
    lo, hi = (0, F1) if form == "latency" else (F - F1, F)       # (the last copy of the batch)
    biggest, g_max, whole = _selection_of(r1 if form == "latency" else r, lo, hi, large)
    assert len(whole) == 6 and min(whole) > 10_000, whole
    assert F1 >= 12 + 10
    _record(3, F1 if form == "latency" else F, form, "shipped", np.array([biggest]))
    print(f", largest g_f {g_max}, whole-image frustums {whole}", end="")


@pytest.mark.parametrize("prm_extra", [{}, {"clamp_bottom": 0}, DEFAULT_QUANTILES, dict(DEFAULT_QUANTILES, clamp_bottom=0)],
                         ids=["params", "params-noclamp", "default-quantiles", "default-quantiles-noclamp"])
def test_large_frustums_quantiles_counts_and_choice(cuda, large, prm_extra):
    from findnpropagate_amd.roiaware_pool3d.roiaware_pool3d_utils import points_in_boxes_count

    sc = large[0]
    head, prm, r1, F1, r, F, n = _large_launches(cuda, large, prm_extra)
    dbg = r1["dbg"]
    H = _host(_cut(r1, 0, F1, 1))
    rows = r1["frustums"].numpy()
    base_corners, mags = head.base_corners.numpy(), head.mags.numpy()
    near = 0
    for f in range(F1):
        m, cam, box, label = int(H["npts"][f]), int(rows[f, 1]), rows[f, 2:6], int(rows[f, 6])
        if m == 0:
            assert H["out_valid"][f] == 0 and H["out_best"][f] == -1 and not H["out_box"][f].any() and H["out_score"][f] == 0
            continue
        uvd, xyz_d = dbg["points_uvd"][f, :m].cpu().numpy(), dbg["points_xyz"][f, :m]
        xyz = xyz_d.cpu().numpy()
        # quantiles -> frustum corners, from the kernel's own depth list and the exact extent of its own lidar-frame points
        fr, wc, _ = SP.restated_frustum(uvd[:, 2], xyz.min(0), xyz.max(0), box, sc, cam, prm)
        SP.check_frustum(H["frust"][f], fr)
        # per-candidate counts: the project's own point-in-box operator on the same points and boxes
        ids = np.nonzero(H["valid"][f] == 2)[0]
        if len(ids):
            want = points_in_boxes_count(xyz_d.contiguous(), dbg["cand"][f][torch.from_numpy(ids).to(cuda)].contiguous())
            SP.check_counts(H["count"][f], H["valid"][f], want.cpu().numpy())
        # choice: the argmax of the second-stage score restated in float64
        s = SP.restated_scores(H["frust"][f], wc, base_corners[label - 1], mags, H["valid"][f], H["iou"][f], H["count"][f], prm)
        best = int(H["out_best"][f])
        near += SP.check_choice(best, s)
        assert H["out_valid"][f] == int(len(ids) > 0)
        if len(ids):
            assert np.array_equal(H["out_box"][f], H["cand"][f][best]) and abs(float(H["out_score"][f]) - s[best]) <= 1e-4
        else:
            assert not H["out_box"][f].any() and H["out_score"][f] == 0
    assert near <= F1 // 10, f"{near} of {F1} frustums have their two best candidates within 1e-4: change the scene"
    assert H["out_valid"].sum() >= F1 // 2
    # the throughput form, copy by copy: the same bits
    one = _cut(r1, 0, F1, 1)
    for b, (lo, hi) in enumerate(_scene_ranges(r, 1, n)):
        _assert_same_scene(_cut(r, lo, hi, 1), one, f"copy {b} of {n} (throughput form) vs the scene alone")
    _record(3, F, "latency (alone, %d) and throughput" % F1, "shipped", H["npts"])
    print(f", near-tied choices {near} of {F1}", end="")


# ---- 4: scene sizes at the trips of the point scan, empty scenes --------------------------------------------------------------
SIZES = [0, 1, 255, 256, 257, 1023, 0, 1024, 1025, 4095, 4096, 4097, 0]      # rows per scene; empty at the first, a middle, the last index


@pytest.fixture(scope="module")
def sized(cuda):
    base = syn.make_seeker_scene(0)
    rng = np.random.default_rng(4)
    scenes = []
    for n in SIZES:
        sc = dict(base)
        sc["points"] = base["points"][np.sort(rng.choice(base["points"].shape[0], n, replace=False))]
        scenes.append(sc)
    alone = []
    for sc in scenes:
        if sc["points"].shape[0] == 0:      # (a launch needs a point tensor: the empty scene's values are stated in the test instead)
            alone.append(None)
            continue
        bd, dets = _batch([sc], cuda)
        r, F, TK = _launch(_head(lambda _, dets=dets: dets), bd, "latency")
        alone.append(_cut(r, 0, F, TK))
    return scenes, alone


@pytest.mark.parametrize("form", ["latency", "throughput"])
def test_scene_sizes_at_the_trip_boundaries_and_empty_scenes(cuda, sized, form):
    scenes, alone = sized
    F0 = alone[1]["npts"].shape[0]      # (every scene carries the same detections)
    F13 = F0 * len(SIZES)
    tiles = 1 if form == "latency" else math.ceil((SEEKER_LAT_MAX_FRUSTUMS + 1) / F13)
    bd, dets = _batch(scenes * tiles, cuda)
    r, F, TK = _launch(_head(lambda _: dets), bd, form)
    assert F == F13 * tiles
    _record(4, F, form, "shipped", r["dbg"]["npts"].cpu().numpy())
    rows = r["frustums"].numpy()
    for b, (lo, hi) in enumerate(_scene_ranges(r, TK, len(SIZES) * tiles)):
        sc, one = scenes[b % len(SIZES)], alone[b % len(SIZES)]
        S = _cut(r, lo, hi, TK)
        assert hi - lo == F0 > 0
        H = _host(S)
        for f in range(lo, hi):      # npts against the float64 count (off by at most the grazing points)
            inside, graze = SP.selection64(SP.project64(sc["points"][:, 1:4], sc, int(rows[f, 1])), rows[f, 2:6])
            assert abs(int(H["npts"][f - lo]) - int(inside.sum())) <= int(graze.sum()), (b, f)
        if one is None:
            assert not H["npts"].any() and not H["out_valid"].any() and (H["out_best"] == -1).all()
            assert not H["out_box"].any() and not H["out_score"].any() and not H["out_count"].any()
        else:
            _assert_same_scene(S, one, f"scene {b} ({sc['points'].shape[0]} rows) in the batch vs alone")


# ---- 5: extraction across the bound ----------------------------------------------------------------------------------------
def test_extraction_of_48_scenes_per_step_equals_2_per_step(cuda, nccl_world1):
    from findnpropagate_amd import extract as E
    from test_gpu_extract import _head as extract_head, _load

    data = syn.SeekerScenes(48, 16, cuda, seed0=0)
    head = extract_head()
    F = head.enumerate_frustums(E.collate_scenes([data[i] for i in range(48)])).shape[0]
    assert F > SEEKER_LAT_MAX_FRUSTUMS
    with tempfile.TemporaryDirectory() as d48, tempfile.TemporaryDirectory() as d2:
        r48, r2 = {}, {}
        assert E.extract_pseudo_labels(data, head, d48, cuda, dist=nccl_world1, recall=r48, scenes_per_step=48) == 48
        assert E.extract_pseudo_labels(data, head, d2, cuda, dist=nccl_world1, recall=r2, scenes_per_step=2) == 48
        a, b = _load(d48), _load(d2)
        assert sorted(a) == sorted(b) == sorted(f"synthetic-{i:06d}_pcd_bin.pth" for i in range(48))
        for f in a:
            for k in a[f]:
                assert torch.equal(a[f][k], b[f][k]), (f, k)
        assert sum(v["pred_boxes"].shape[0] for v in a.values()) > 48 * 5
    assert r48 == r2 and r48["gt"] > 0 and 0 < r48["rcnn_0.3"] <= r48["gt"]
    _record(5, F, "throughput", "shipped (extract_pseudo_labels, 48 scenes per step)", None)
