"""tests/ref_box.py against the CPU oracle, without a GPU: the inputs of tests/test_gpu_box_at_scale.py have the structure the
device code has never met (suppressors 65 and more column words away, a partial last word, exact duplicates at threshold 1.0), the
undecided band is as wide as measured, and every checker FAILS on a planted defect of the kind it is there to find."""
import numpy as np
import pytest

import ref_box as R

FAR_BOXES_AT_4800 = 30


def _sweep(mask, n, reach=None, ones_from=None, drop_partial=False):
    """host_sweep with the planted sweep defects: `reach` = a kept box updates only the words bi + 1 .. bi + reach (the update
    loop's first trip), `ones_from` = remv[ones_from:] starts as all-ones (the init loop's first trip only), `drop_partial` = the
    last, partial word is never visited."""
    cb = R.words(n)
    remv = np.zeros((cb,), np.uint64)
    if ones_from is not None:
        remv[ones_from:] = ~np.uint64(0)
    rows = n - n % 64 if drop_partial else n
    keep = []
    for i in range(rows):
        w = i >> 6
        if not (remv[w] >> np.uint64(i & 63)) & np.uint64(1):
            keep.append(i)
            hi = cb if reach is None else min(cb, w + 1 + reach)
            remv[w:hi] |= mask[i, w:hi]
    return np.array(keep, np.int64)


def _cases(flavour):
    return R.rotated_case if flavour == "rotated" else R.normal_case


# ---------------------------------------------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("n", R.NMS_SIZES)
def test_band_is_four_times_the_measured_heading_sensitivity(oracle, n):
    boxes, pairs, _ = R.rotated_pairs(n)
    s = R.heading_sensitivity(boxes, pairs)
    print(f"FORM band n {n} candidates {len(pairs)} max |dIoU| for 4 ulps of heading {s:.3e} x4 {4 * s:.3e} BAND {R.BAND:.1e}")
    assert 0 < 4 * s <= R.BAND
    assert s >= R.BAND / 40, "BAND is far wider than measured: measure again"


@pytest.mark.parametrize("n,thresh", R.NMS_CASES)
def test_rotated_inputs_meet_the_conditions(oracle, n, thresh):
    c = R.rotated_case(n, thresh)
    over, und, kept = int(c["over"].sum()), int(c["undecided"].sum()), len(c["keep"])
    near, dist = R.nearest_suppressor_words(c["mask"], c["keep"], n)
    far = int((near >= 65).sum())
    print(f"FORM inputs rotated n {n} words {R.words(n)} thresh {thresh} candidates {len(c['pairs'])} over {over} undecided {und} "
          f"({und / max(over, 1):.4%}) kept {kept} ({kept / n:.1%}) boxes with every kept suppressor >= 65 words away {far} "
          f"suppressions across exactly 64 words {int((dist == 64).sum())}")
    assert und <= R.UNDECIDED_SHARE_CAP * over
    _structure(n, thresh, kept, far, dist)


@pytest.mark.parametrize("n,thresh", R.NMS_CASES)
def test_axis_aligned_inputs_meet_the_conditions(n, thresh):
    c = R.normal_case(n, thresh)
    kept = len(c["keep"])
    near, dist = R.nearest_suppressor_words(c["mask"], c["keep"], n)
    far = int((near >= 65).sum())
    print(f"FORM inputs normal n {n} words {R.words(n)} thresh {thresh} kept {kept} ({kept / n:.1%}) far {far} across 64 {int((dist == 64).sum())}")
    assert R.check_mask_shape(c["mask"], n, c["pairs"]) == dict(non_candidate=0, past_n=0)   # the candidate argument holds
    _structure(n, thresh, kept, far, dist)


def _structure(n, thresh, kept, far, dist):
    if thresh == 1.0:
        assert kept == n                      # nothing is "> 1.0", the exact duplicates included
        return
    assert 0.10 * n <= kept <= 0.70 * n
    if n >= 4161:
        assert far >= 1
    if n == 4800:
        assert far >= FAR_BOXES_AT_4800
    if R.words(n) >= 65:
        assert (dist == 64).any()


def test_planted_rows(oracle):
    for n in R.NMS_SIZES:
        b = R.make_boxes(n)
        d = R.duplicate_pairs(n)
        assert np.array_equal(b[d[:, 0]], b[d[:, 1]]) and (b[d[:, 0], 6] == 0).all()
        assert np.array_equal(b[:R.N_EXACT, :6] * 4, np.round(b[:R.N_EXACT, :6] * 4))
        assert d[0].tolist() == [0, n - 1] and (d[:, 1] >> 6).min() >= R.words(n) - 2
        # the oracle's IoU of an exact duplicate is exactly 1.0: decided at every threshold, and not "> 1.0"
        assert (R.iou_rotated(b, d) == np.float32(1.0)).all()
        assert [float(h) for h in b[8:13, 6]] == [float(np.float32(h)) for h in R.EXACT_HEADINGS]
        special = np.array([[13, n - 10], [14, n - 9]])
        pairs = R.candidates(b)
        have = set(map(tuple, pairs.tolist()))
        assert all(tuple(p) in have for p in special.tolist() + d.tolist())
        iou = R.iou_rotated(b, special)
        assert iou[0] == 0 and 0.01 < iou[1] < 0.011      # touching: no area; nested: 1.05 / 100
    assert R.make_boxes(65).shape == (65, 7) and R.make_boxes(4800) is R.make_boxes(4800)


def test_non_candidates_do_not_overlap(oracle, rng):
    """the candidate argument, sampled: the oracle's overlap of pairs left out is exactly 0"""
    b = R.make_boxes(4800)
    have = R.candidates(b)
    key = set((have[:, 0] * 4800 + have[:, 1]).tolist())
    i = rng.integers(0, 4800, 60000)
    j = rng.integers(0, 4800, 60000)
    m = (i < j) & np.array([a * 4800 + c not in key for a, c in zip(i.tolist(), j.tolist())])
    p = np.stack([i[m], j[m]], 1)
    # and the nearest misses among the first 600 rows: clearance between 0.1 m (the candidates' limit) and 0.5 m
    bb = b[:600].astype(np.float64)
    rad = np.hypot(bb[:, 3], bb[:, 4]) / 2
    clear = np.hypot(bb[:, None, 0] - bb[None, :, 0], bb[:, None, 1] - bb[None, :, 1]) - rad[:, None] - rad[None, :]
    near = np.stack(np.nonzero(np.triu((clear > 0.1) & (clear < 0.5), 1)), 1)
    assert not any(r[0] * 4800 + r[1] in key for r in near.tolist())
    assert len(p) > 20000 and len(near) > 10
    assert (R.iou_rotated(b, np.concatenate([p, near])) == 0).all()


# ---------------------------------------------------------------------------------------------------------------- planted defects
@pytest.mark.parametrize("flavour", ["rotated", "normal"])
@pytest.mark.parametrize("n,thresh", R.NMS_CASES)
def test_planted_sweep_defects_change_the_result(oracle, flavour, n, thresh):
    c = _cases(flavour)(n, thresh)
    mask, keep, cb = c["mask"], c["keep"], R.words(n)
    assert np.array_equal(_sweep(mask, n), keep)
    if cb >= 66 and thresh < 1.0:       # the update loop's second trip lost: row n-1 (n = 4161) is kept although row 0 suppresses it
        assert not np.array_equal(_sweep(mask, n, reach=64), keep)
    else:                               # up to 65 words the first trip reaches everything (threshold 1.0: nothing to suppress)
        assert np.array_equal(_sweep(mask, n, reach=64), keep)
    if cb >= 65 and thresh < 1.0:       # the first trip one word short: the suppression across exactly 64 words is lost
        assert not np.array_equal(_sweep(mask, n, reach=63), keep)
    # the last word of n = 4097 and of n = 4161 holds ONE row, row 0's duplicate: the one box 64 / 65 words from its only kept
    # suppressor, so suppressed below threshold 1.0.  Defects that wrongly REMOVE boxes of the late words therefore show where
    # those words hold kept boxes: word 64 of n = 4161, words 64 .. 74 of n = 4800, and everywhere at threshold 1.0.
    late_kept = bool((keep >= 4096).any())
    assert late_kept == (n >= 4161)
    if late_kept:                       # the init loop's second trip lost
        assert not np.array_equal(_sweep(mask, n, ones_from=64), keep)
    partial_kept = bool(n % 64) and bool((keep >= n - n % 64).any())
    assert partial_kept == ((n, thresh) == (4161, 1.0))
    if partial_kept:
        assert not np.array_equal(_sweep(mask, n, drop_partial=True), keep)


@pytest.mark.parametrize("n,thresh", [(4096, 0.1), (4161, 0.7), (4800, 0.1)])
def test_a_flipped_bit_outside_the_band_is_found(oracle, rng, n, thresh):
    c = R.rotated_case(n, thresh)
    clean = R.check_mask_rotated(c["mask"], c)
    assert clean == dict(non_candidate=0, past_n=0, decided_wrong=0, undecided_differ=0)
    decided = np.nonzero(~c["undecided"])[0]
    for k in rng.choice(decided, 5, replace=False).tolist() + [int(np.nonzero(~c["undecided"] & c["over"])[0][-1])]:
        i, j = c["pairs"][k]
        m = c["mask"].copy()
        m[i, j >> 6] ^= np.uint64(1) << np.uint64(j & 63)
        assert R.check_mask_rotated(m, c)["decided_wrong"] == 1
        cn = R.normal_case(n, thresh)
        mn = cn["mask"].copy()
        mn[i, j >> 6] ^= np.uint64(1) << np.uint64(j & 63)
        assert R.check_mask_normal(mn, cn)["words_differ"] == 1
    if c["undecided"].any():            # a flip INSIDE the band is counted, not failed
        i, j = c["pairs"][np.nonzero(c["undecided"])[0][0]]
        m = c["mask"].copy()
        m[i, j >> 6] ^= np.uint64(1) << np.uint64(j & 63)
        r = R.check_mask_rotated(m, c)
        assert r["decided_wrong"] == 0 and r["undecided_differ"] == 1
    m = c["mask"].copy()
    m[0, R.words(n) - 1] |= np.uint64(1) << np.uint64(63 if n % 64 else 5)      # a column past n, or a far-away non-candidate
    r = R.check_mask_rotated(m, c)
    assert r["non_candidate"] == 1 and r["past_n"] == (1 if n % 64 else 0)


def test_greater_or_equal_is_found_on_the_duplicates_at_threshold_one(oracle):
    n = 4161
    c = R.rotated_case(n, 1.0)
    dup = R.duplicate_pairs(n)
    ge = R.mask_from_pairs(n, c["pairs"], c["iou"] >= np.float32(1.0))
    assert R.get_bits(ge, dup).all() and not R.get_bits(c["mask"], dup).any() and not c["undecided"].any()
    assert R.check_mask_rotated(ge, c)["decided_wrong"] >= len(dup)
    assert len(R.host_sweep(ge, n)) <= n - len(dup) and len(c["keep"]) == n
    cn = R.normal_case(n, 1.0)
    gen = R.mask_normal(cn["boxes"], 1.0, ge=True)
    assert R.get_bits(gen, dup).all() and R.check_mask_normal(gen, cn)["words_differ"] >= len(dup)
    assert len(R.host_sweep(gen, n)) <= n - len(dup) and len(cn["keep"]) == n


def test_batched_decode_with_the_row_stride_of_cap_is_found():
    cap, counts = 4800, [4800, 4161, 4096, 65, 0]
    masks = [R.normal_case(c, 0.1)["mask"] if c >= 4096 else R.mask_normal(R.make_boxes(c), 0.1) if c else np.zeros((0, 0), np.uint64)
             for c in counts]
    ws = np.full((len(counts) * cap * R.words(cap),), ~np.uint64(0), np.uint64)     # the layout fnp_nms_batched writes
    for z, m in enumerate(masks):
        ws[z * cap * R.words(cap):][: m.size] = m.ravel()
    got = R.decode_ws_batched(ws.view(np.uint8), cap, counts)
    for z, c in enumerate(counts):
        assert np.array_equal(got[z], masks[z])
        if c:
            assert np.array_equal(R.decode_ws(ws[z * cap * R.words(cap):], c), masks[z])
    for z, c in enumerate(counts[1:4], 1):       # the defect: rows taken ceil(cap / 64) words apart
        base = z * cap * R.words(cap)
        wrong = ws[base: base + c * R.words(cap)].reshape(c, R.words(cap))[:, : R.words(c)]
        assert not np.array_equal(wrong, masks[z])
        assert not np.array_equal(R.host_sweep(wrong, c), R.host_sweep(masks[z], c))


# ---------------------------------------------------------------------------------------------------------------- restatements
@pytest.mark.parametrize("n,thresh", [(700, 0.1), (4161, 0.1), (4161, 1.0), (4800, 0.7)])
def test_host_sweep_over_the_oracles_mask_is_oracle_nms(oracle, n, thresh):
    for rotated in (True, False):
        c = (R.rotated_case if rotated else R.normal_case)(n, thresh)
        assert np.array_equal(c["keep"], oracle.nms(c["boxes"], thresh, rotated))
        assert np.array_equal(c["keep"], _sweep(c["mask"], n))


def test_mask_normal_is_the_oracles_axis_aligned_iou(oracle, rng):
    n = 4161
    b = R.make_boxes(n)
    pairs = R.candidates(b)
    sample = np.concatenate([pairs[rng.choice(len(pairs), 3000, replace=False)], R.duplicate_pairs(n),
                             np.sort(rng.integers(0, n, (500, 2)), axis=1)])
    sample = sample[sample[:, 0] < sample[:, 1]]
    iou = np.array([oracle.iou_normal(b[i], b[j]) for i, j in sample.tolist()], np.float32)
    for thresh in (0.1, 0.7, 1.0):
        assert np.array_equal(R.get_bits(R.normal_case(n, thresh)["mask"], sample), iou > np.float32(thresh))
    assert (iou > 0.7).sum() > 50 and (iou == 0).sum() > 300


def test_iou3d_from_overlap_is_the_oracles(oracle):
    A, B, a2, b2 = R.pairwise_inputs()
    assert np.array_equal(R.iou3d_from_overlap(A, B, oracle.boxes_overlap_bev(A, B)), oracle.boxes_iou3d(A, B))
    al = R.iou3d_from_overlap(a2, b2, oracle.boxes_aligned_overlap_bev(a2, b2))
    assert np.array_equal(al[:277], np.diagonal(oracle.boxes_iou3d(a2[:277], b2[:277]))) and (al > 0.3).sum() > 1000


# ---------------------------------------------------------------------------------------------------------------- the other inputs
def test_pairwise_inputs(oracle):
    """no pair of the pairwise matrices sits on a discontinuity of the overlap (a corner entering the 1e-2 margin, a crossing
    appearing): 4 ulps of heading move no IoU by more than BAND / 4, so the float tolerances of the GPU test are about rounding"""
    A, B, a2, b2 = R.pairwise_inputs()
    assert A.shape == (531, 7) and B.shape == (277, 7) and a2.shape == b2.shape == (10001, 7)
    cp = R.cross_pairs(A, B)
    s = R.heading_sensitivity(np.concatenate([A, B]), np.stack([cp[:, 0], cp[:, 1] + 531], 1))
    k = np.arange(10001)
    s2 = R.heading_sensitivity(np.concatenate([a2, b2]), np.stack([k, k + 10001], 1))
    iou = oracle.boxes_iou_bev(A, B)
    print(f"FORM inputs pairwise candidates {len(cp)} overlapping {(iou > 0).sum()} sensitivity {s:.3e} aligned {s2:.3e}")
    assert 4 * max(s, s2) <= R.BAND and (iou > 0).sum() > 3000 and (iou > 0.5).sum() > 100
    out = np.ones(iou.shape, bool)
    out[cp[:, 0], cp[:, 1]] = False
    assert (iou[out] == 0).all()


def test_recall_inputs_have_no_best_iou_within_the_band(oracle):
    gt, preds, rois, garbage = R.recall_inputs()
    G = R.RECALL_GT
    assert gt.shape == (G + R.RECALL_PAD, 10) and preds.shape == (R.RECALL_PREDS, 7) and rois.shape == (R.RECALL_ROIS, 7)
    assert not gt[G:].any() and not gt[list(R.RECALL_ZERO_ROWS)].any() and gt[G - 1].any() and len(R.RECALL_THRESH) == 8
    thr = np.array(R.RECALL_THRESH, np.float32).astype(np.float64)
    best = oracle.boxes_iou3d(preds, gt[:G, :7]).max(0)
    best_roi = oracle.boxes_iou3d(rois, gt[:G, :7]).max(0)
    d = min(np.abs(best[:, None] - thr).min(), np.abs(best_roi[:, None] - thr).min())
    pi, gi = np.nonzero(oracle.boxes_iou3d(preds, gt[:G, :7]) > 0)
    s = R.heading_sensitivity(np.concatenate([preds, gt[:G, :7]]), np.stack([pi, gi + len(preds)], 1), iou_fn=R.iou3d_aligned_oracle)
    hits = [(best > t).sum() for t in thr]
    print(f"FORM inputs recall nearest best IoU to a threshold {d:.3e} sensitivity {s:.3e} hits per threshold {hits}")
    assert d >= R.BAND and 4 * s <= R.BAND
    assert hits[0] > hits[3] > hits[-1] > 20 and (oracle.boxes_iou3d(garbage[None], gt[:G, :7]) > 0.8).any()


def test_point_in_box_inputs_reach_every_tile(oracle):
    boxes, pts = R.pib_inputs()
    assert boxes.shape == (R.PIB_T, 7) and pts.shape == (R.PIB_M, 3)
    first = oracle.points_in_boxes(pts[None], boxes[None])[0]
    in2 = oracle.points_in_boxes(pts[None], boxes[None, 128:256])[0] >= 0
    in3 = oracle.points_in_boxes(pts[None], boxes[None, 256:])[0] >= 0
    n12, n23, n3 = ((first >= 0) & (first < 128) & in2).sum(), ((first >= 128) & (first < 256) & in3).sum(), (first == 256).sum()
    print(f"FORM inputs points-in-boxes first box in tile 1 and tile 2 holds it too {n12}, in tile 2 and tile 3 too {n23}, in tile 3 {n3}")
    assert min(n12, n23, n3) > 100 and (first < 0).sum() > 1000
