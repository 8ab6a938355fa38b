"""sparse.rows_in_boxes (fnp_rows_in_boxes): the rows of a batch inside boxes, compact, against the host form
(augmentor.pseudo_loader.points_in_boxes_compact -> fnp_host_points_in_boxes_compact) scene by scene: the counts, the
scene-relative indices and the raw rows, all equal (the membership test has no tolerance: same expressions, same bits)."""
import numpy as np
import pytest
import torch

from findnpropagate_amd import sparse as S
from findnpropagate_amd import synthetic as syn
from findnpropagate_amd.augmentor import database_sampler as DS
from findnpropagate_amd.augmentor.pseudo_loader import points_in_boxes_compact
from test_gpu_gt_sampling import sampled_boxes

pytestmark = pytest.mark.gpu
PAD_ROWS = 300        # rows behind batch_offsets[B], as the assembly leaves them


def host(scenes, boxes, cuts=None):
    """per scene the host form -> (counts (T,), indices (K,), rows (K, 5)) of the batch, box after box"""
    counts, idx, rows = [], [], []
    for b, (sc, bx) in enumerate(zip(scenes, boxes)):
        cut = None if cuts is None else (DS.cut_records(cuts[b][0]), cuts[b][1], cuts[b][2])
        c, i, _ = points_in_boxes_compact(sc, bx, cut=cut)
        counts.append(c)
        idx.append(i)
        rows.append(sc[i])
    return np.concatenate(counts), np.concatenate(idx).astype(np.int32), np.concatenate(rows, 0).astype(np.float32)


def device_args(scenes, boxes, cuts, dev):
    pts = np.concatenate(list(scenes) + [np.full((PAD_ROWS, 5), S.PREP_PAD, np.float32)], 0)
    off = np.concatenate([[0], np.cumsum([s.shape[0] for s in scenes])]).astype(np.int32)
    box_off = np.concatenate([[0], np.cumsum([b.shape[0] for b in boxes])]).astype(np.int32)
    rec = DS.cut_records(np.concatenate(boxes, 0))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cut = None
    if cuts is not None:
        cut = (t(DS.cut_records(np.concatenate([c[0] for c in cuts], 0))),
               t(np.concatenate([[0], np.cumsum([c[0].shape[0] for c in cuts])]).astype(np.int32)),
               t(np.array([c[1] for c in cuts], np.int32)), t(np.array([c[2] for c in cuts], np.int32)))
    return (t(pts), t(off), len(scenes), t(rec), t(box_off)), cut


def check(scenes, boxes, cuts, dev, capacity=None):
    want_c, want_i, want_r = host(scenes, boxes, cuts)
    total = int(want_c.sum())
    args, cut = device_args(scenes, boxes, cuts, dev)
    cap = total + 5 if capacity is None else capacity
    res = S.rows_in_boxes(*args, cut=cut, capacity=cap)
    assert np.array_equal(res["counts"].cpu().numpy(), want_c) and int(res["total"].item()) == total
    k = min(cap, total)
    assert np.array_equal(res["indices"].cpu().numpy()[:k], want_i[:k])
    assert np.array_equal(res["rows"].cpu().numpy()[:k].view(np.uint32), want_r[:k].view(np.uint32))
    c, i, r = S.rows_in_boxes_exact(*args, cut=cut, capacity=cap)
    assert c.dtype == np.int64 and np.array_equal(c, want_c) and np.array_equal(i, want_i)
    assert np.array_equal(r.view(np.uint32), want_r.view(np.uint32))
    return want_c


def rows(rng, n, lo=-20, hi=20):
    p = rng.uniform(lo, hi, (n, 5)).astype(np.float32)
    p[:, 2] = rng.uniform(-3, 2, n)
    return p


def batch():
    """3 scenes with 0 / 1 / 37 boxes.  Scene 2 starts at batch row 1000: its rows 24 ... 279 are the 256-row block 4 of the
    batch and all lie in box 3 of the scene; box 4 holds no row; box 5, at the origin with heading 0, has rows exactly on its
    faces, one step inside and one step outside, and no other; rows at the block borders 1535 | 1536 and 1791 | 1792 lie in
    box 6"""
    rng = np.random.default_rng(808)
    s0, s1, s2 = rows(rng, 613), rows(rng, 387), rows(rng, 3000)
    b1 = syn.random_boxes(rng, 1, centre_range=5.0)
    b1[:, 3:6] = 9.0
    b2 = syn.random_boxes(rng, 37, centre_range=15.0)
    b2[3] = [40, 40, 0, 2, 2, 2, 0.4]
    s2[24:280, :3] = np.array([40, 40, 0], np.float32) + rng.uniform(-0.5, 0.5, (256, 3)).astype(np.float32)
    b2[4] = [-60, 60, 0, 3, 3, 3, 1.0]
    b2[5] = [0, 0, 0, 1, 2, 4, 0.0]
    s2[(np.abs(s2[:, 0]) < 1) & (np.abs(s2[:, 1]) < 2), 0] += 5
    f32 = np.float32
    face = []
    for v in (f32(0.5), np.nextafter(f32(0.5), f32(0)), np.nextafter(f32(0.5), f32(1))):
        face += [(v, 0, 0), (-v, 0, 0), (0, 2 * v, 0), (0, -2 * v, 0), (0, 0, 4 * v), (0, 0, -4 * v)]
    s2[400:400 + len(face), :3] = np.array(face, np.float32)
    b2[6] = [-45, -45, 0, 4, 4, 4, -2.0]
    for r in (535, 536, 791, 792):
        s2[r, :3] = np.array([-45, -45, 0], np.float32) + rng.uniform(-0.3, 0.3, 3).astype(np.float32)
    return [s0, s1, s2], [np.zeros((0, 7), np.float32), b1, b2]


def test_batch_matches_host(cuda):
    scenes, boxes = batch()
    counts = check(scenes, boxes, None, cuda)
    c2 = counts[1:]
    assert c2[3] == 256 and c2[4] == 0 and c2[6] == 4 and counts[0] > 0
    assert c2[5] == 12                                       # on the face and one step inside: in; one step outside: out
    total = int(counts.sum())
    # capacity below the total: the counts are complete, the first rows right, and the retry is exact
    for cap in (0, 1, 255, total - 1, total):
        check(scenes, boxes, None, cuda, capacity=cap)
    # a pending cut whose windows start and end inside a wave; scene 2's cut boxes are copies of some of its boxes
    cuts = [(syn.random_boxes(np.random.default_rng(1), 3), 0, 10 ** 6), (boxes[1].copy(), 37, 301),
            (np.concatenate([boxes[2][[3, 6, 10, 11]], syn.random_boxes(np.random.default_rng(2), 5)]), 24 + 70, 24 + 256 - 27)]
    cut_counts = check(scenes, boxes, cuts, cuda)
    assert cut_counts[1 + 3] == 70 + 27 and 0 < cut_counts[0] < counts[0]
    check(scenes, boxes, cuts, cuda, capacity=100)
    # no cut records at all is no cut
    none = [(np.zeros((0, 7), np.float32), 0, 10 ** 6)] * 3
    assert np.array_equal(check(scenes, boxes, none, cuda), counts)


def test_no_boxes_and_empty_scenes(cuda):
    scenes, boxes = batch()
    empty = [np.zeros((0, 7), np.float32)] * 3
    args, _ = device_args(scenes, empty, None, cuda)
    res = S.rows_in_boxes(*args, capacity=16)
    assert res["counts"].numel() == 0 and int(res["total"].item()) == 0
    c, i, r = S.rows_in_boxes_exact(*args, capacity=16)
    assert c.shape == (0,) and i.shape == (0,) and r.shape == (0, 5)
    # an empty scene that has boxes, between two scenes; then scenes without any row
    none = np.zeros((0, 5), np.float32)
    counts = check([scenes[1], none, scenes[2]], [boxes[1], boxes[2][:5], boxes[2]], None, cuda)
    assert counts[1:6].sum() == 0 and counts[6:].sum() > 0
    counts = check([none, none], [boxes[1], boxes[2][:3]], None, cuda)
    assert counts.sum() == 0
    global PAD_ROWS
    keep, PAD_ROWS = PAD_ROWS, 0
    try:
        assert check([none, none], [boxes[1], boxes[2][:3]], None, cuda).sum() == 0            # N == 0
        check(scenes, boxes, None, cuda)                                                       # no pad rows behind the batch
    finally:
        PAD_ROWS = keep


def test_ten_sweep_scenes_with_40_boxes(cuda):
    pts, o = syn.make_sweeps_batch([0, 1, 2, 3])
    rng = np.random.default_rng(809)
    scenes = [pts[o[b]:o[b + 1]] for b in range(4)]
    boxes = [sampled_boxes(rng, 40, s) for s in scenes]
    cuts = [(sampled_boxes(rng, 39, s), 2000, s.shape[0] - 1500) for s in scenes]
    assert check(scenes, boxes, None, cuda).sum() > 4000
    check(scenes, boxes, cuts, cuda, capacity=4096)
