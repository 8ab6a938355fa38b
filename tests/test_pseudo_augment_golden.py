"""DataAugmentor's pseudo-label entries (load_frustum_pseudos, load_selftrain_pseudos, unknowns_copy_paste) against the
reference's own DataAugmentor (tests/golden/pseudo_augment_golden.npz, made by tests/golden/make_pseudo_augment_golden.py),
frame after frame of one augmentor per case, bit for bit; the deferred mode (pending cut, prep_cut_to) against the host mode;
the compact membership (fnp_host_points_in_boxes_compact) against the dense one.  CPU only."""
import os
import pickle
from pathlib import Path

import numpy as np
import pytest

import pseudo_augment_scenario as SC
from findnpropagate_amd import lib
from findnpropagate_amd import synthetic as syn
from findnpropagate_amd.augmentor import data_augmentor as DA
from findnpropagate_amd.augmentor import database_sampler as DS
from findnpropagate_amd.augmentor import pseudo_loader as PL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pseudo_augment_golden.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def scenario(tmp_path_factory, golden):
    root, fr, st = (tmp_path_factory.mktemp(n) for n in ("db", "frustum", "selftrain"))
    for db, sha in SC.write_databases(str(root)).items():
        assert sha == str(golden[f"db_sha256/{db}"]), f"database {db} drifted from the golden's"
    return root, str(fr), str(st), SC.make_frames(str(fr), str(st))


def next_draw():
    st = np.random.get_state()
    v = np.random.random()
    np.random.set_state(st)
    return v


def augmentor(case, scenario, deferred=False):
    root, fr, st, _ = scenario
    return DA.DataAugmentor(Path(root), SC.augmentor_config(case, fr, st), SC.CLASS_NAMES, deferred=deferred)


def apply_pending(d):
    """the device's work on the host: the cut window, then the program (host-mode arithmetic)"""
    pts = np.asarray(d["points"], np.float32)
    if DS.CUT_BOXES_KEY in d:
        lo, hi = d[DS.CUT_FROM_KEY], d.get(DA.CUT_TO_KEY, pts.shape[0])
        keep = np.ones(pts.shape[0], bool)
        keep[lo:hi] = DS.points_outside_boxes(pts[lo:hi], DS.cut_records(d[DS.CUT_BOXES_KEY]))
        pts = pts[keep]
    for op, a, b, c in d.get(DA.PROGRAM_KEY, np.zeros((0, 4), np.float32)):
        pts = pts.copy()
        if op == DA.OP_FLIP_X:
            pts[:, 1] = -pts[:, 1]
        elif op == DA.OP_FLIP_Y:
            pts[:, 0] = -pts[:, 0]
        elif op == DA.OP_ROTATE:
            x, y = pts[:, 0].copy(), pts[:, 1].copy()
            pts[:, 0] = DA._fma32(y, -b, x * a)
            pts[:, 1] = DA._fma32(y, a, x * b)
        elif op == DA.OP_SCALE:
            pts[:, :3] *= a
        elif op == DA.OP_TRANSLATE:
            pts[:, :3] += np.array([a, b, c], np.float32)
    return pts


def queue_state(aug):
    q = aug.pseudo_loader.sampler.unknown_queue
    return [[(o.points.tobytes(), o.box.tobytes(), float(o.conf), o.x, o.y, o.z, o.ry) for o in q[l]] for l in sorted(q)]


def check(golden, key, out, draw):
    for k in ("points", "gt_boxes", "pseudo_boxes", "pseudo_samples_mask"):
        got, exp = np.asarray(out[k]), golden[f"{key}/{k}"]
        assert got.dtype == exp.dtype and got.shape == exp.shape, (key, k, got.dtype, exp.dtype, got.shape, exp.shape)
        assert np.array_equal(got, exp), (key, k)
    assert np.array_equal(np.asarray(out["gt_names"]).astype(str), golden[f"{key}/gt_names"]), key
    assert draw == golden[f"{key}/next_draw"], key
    assert "pseudo_scores" not in out


@pytest.mark.parametrize("case", list(SC.CASES))
def test_host_mode_matches_reference(golden, scenario, case):
    np.random.seed(SC.seed_of(case))
    aug = augmentor(case, scenario)
    for k, frame in enumerate(scenario[3]):
        out = aug.forward(SC.data_dict(frame))
        check(golden, f"{case}/{k}", out, next_draw())
    q = aug.pseudo_loader.sampler.unknown_queue
    assert np.array_equal([len(q[l]) for l in aug.pseudo_loader.unknown_class_labels], golden[f"{case}/queue_sizes"])


def test_golden_exercises_the_cases(golden):
    assert sum(int(golden[f"{c}/{k}/pseudo_samples_mask"].sum()) for c in SC.CASES for k in range(SC.N_FRAMES)) > 20
    assert golden["num_pts/queue_sizes"].max() == 2                  # a full queue: entries were replaced
    assert not np.array_equal(golden["fix_cp_none/4/points"], golden["shipped/4/points"])


@pytest.mark.parametrize("case", list(SC.CASES))
def test_deferred_mode_gives_host_rows(golden, scenario, case):
    """deferred augmentor + the cut window and the program on the host = host mode, frame by frame; queues and draws equal"""
    np.random.seed(SC.seed_of(case))
    host = augmentor(case, scenario)
    dfr = augmentor(case, scenario, deferred=True)
    for k, frame in enumerate(scenario[3]):
        st = np.random.get_state()
        h = host.forward(SC.data_dict(frame))
        hd = next_draw()
        after = np.random.get_state()
        np.random.set_state(st)
        d = dfr.forward(SC.data_dict(frame))
        assert next_draw() == hd
        np.random.set_state(after)
        for key in ("gt_boxes", "pseudo_boxes", "pseudo_samples_mask"):
            assert np.array_equal(h[key], d[key]), (case, k, key)
        if DS.CUT_BOXES_KEY in d:
            assert d[DA.CUT_TO_KEY] <= d["points"].shape[0]
        assert np.array_equal(apply_pending(d), np.asarray(h["points"], np.float32)), (case, k)
        assert queue_state(host) == queue_state(dfr), (case, k)


def test_overlap_case_pastes_into_cut_boxes(scenario):
    """the overlap sequence has pasted rows inside a cut box; the device must keep them (cut_to stops the window)"""
    np.random.seed(SC.seed_of("overlap"))
    aug = augmentor("overlap", scenario, deferred=True)
    hits = 0
    for frame in scenario[3]:
        d = aug.forward(SC.data_dict(frame))
        lo, hi = d[DS.CUT_FROM_KEY], d[DA.CUT_TO_KEY]
        pasted = np.asarray(d["points"][hi:], np.float32)
        if pasted.shape[0] and d[DS.CUT_BOXES_KEY].shape[0]:
            hits += int((~DS.points_outside_boxes(pasted, DS.cut_records(d[DS.CUT_BOXES_KEY]))).sum())
    assert hits > 0


def dense_ref(points, boxes):
    points = np.ascontiguousarray(points, np.float32)
    boxes = np.ascontiguousarray(boxes[:, :7], np.float32)
    T, (N, C) = boxes.shape[0], points.shape
    in_box = np.zeros((T, N), np.uint8)
    out = np.empty((T, N, C), np.float32)
    rc = lib.load().fnp_host_points_in_boxes_frame(points.ctypes.data if N else None, N, C, boxes.ctypes.data if T else None, T,
                                                    in_box.ctypes.data if T * N else None, out.ctypes.data if T * N else None)
    lib.check(rc, "fnp_host_points_in_boxes_frame")
    return in_box.astype(bool), out


def check_compact(points, boxes, cut=None, keep_rows=None):
    counts, idx, rows = PL.points_in_boxes_compact(points, boxes, cut=cut)
    src = points if keep_rows is None else points[keep_rows]
    inside, frame = dense_ref(src, boxes)
    assert np.array_equal(counts, inside.sum(1))
    t, i = np.nonzero(inside)
    want_idx = i if keep_rows is None else np.nonzero(keep_rows)[0][i]
    assert np.array_equal(idx, want_idx)
    assert rows.dtype == np.float32 and np.array_equal(rows.view(np.uint32), frame[t, i].view(np.uint32))
    return counts


def face_scene(rng, boxes, C):
    """rows on the faces of axis-aligned and rotated boxes (inclusive faces), plus random rows"""
    rows = []
    for b in boxes:
        for sx in (-0.5, 0.0, 0.5):
            for sz in (-0.5, 0.5):
                lx, lz = sx * b[3], sz * b[5]
                c, s = np.cos(b[6]), np.sin(b[6])
                rows.append([b[0] + lx * c, b[1] + lx * s, b[2] + lz])
    p = np.zeros((len(rows) + 500, C), np.float32)
    p[:len(rows), :3] = rows
    p[len(rows):, :3] = rng.uniform(-10, 10, (500, 3))
    p[:, 3:] = rng.uniform(0, 1, (p.shape[0], C - 3))
    return p


@pytest.mark.parametrize("C", [5, 8])
def test_compact_membership_equals_dense(rng, C):
    boxes = syn.random_boxes(rng, 12, centre_range=8.0)
    boxes[:4, 6] = [0.0, np.pi / 2, np.pi, -np.pi / 2]
    pts = face_scene(rng, boxes, C)
    assert check_compact(pts, boxes)[:4].sum() > 0
    check_compact(pts, boxes[:0])                                            # T = 0
    check_compact(pts[:0], boxes)                                            # N = 0
    check_compact(np.tile(pts, (30, 1)), boxes)                              # past the first capacity guess


def test_compact_membership_with_cut_equals_cut_scene(rng):
    pts = face_scene(rng, syn.random_boxes(rng, 3, 8.0), 5)
    pts = np.concatenate([pts, rng.uniform(-6, 6, (3000, 5)).astype(np.float32)])
    boxes = syn.random_boxes(rng, 10, centre_range=6.0)
    cut_boxes = syn.random_boxes(rng, 6, centre_range=6.0)
    rec = DS.cut_records(cut_boxes)
    for lo, hi in ((0, pts.shape[0]), (200, 2500), (300, 300), (0, 2 ** 31 - 1), (pts.shape[0], pts.shape[0] + 5)):
        keep = np.ones(pts.shape[0], bool)
        keep[lo:hi] = DS.points_outside_boxes(pts[lo:hi], rec)
        check_compact(pts, boxes, cut=(rec, lo, hi), keep_rows=keep)
    assert not DS.points_outside_boxes(pts, rec).all()


def test_copy_paste_needs_a_loader():
    with pytest.raises(AttributeError):
        DA.DataAugmentor(None, [SC.EDict(NAME='unknowns_copy_paste', MAX_QUEUE_SIZE=3)], SC.CLASS_NAMES)


def test_selftrain_builds_a_loader_only_once(scenario):
    root, fr, st, _ = scenario
    cfg = SC.augmentor_config("no_gt_sampling", fr, st)
    aug = DA.DataAugmentor(Path(root), cfg, SC.CLASS_NAMES)
    loader = aug.pseudo_loader
    assert loader.sampler.max_queue_size_per_class == 60 and loader.sampler.queue_metric == 'conf'
    assert loader.fix_cp == 10 and loader.copy_st_only and not loader.sampler.validate_pseudos and loader.mom == 0.9997
    only = DA.DataAugmentor(Path(root), [SC.EDict(NAME='load_selftrain_pseudos', KNOWN_CLASSES=SC.KNOWN, PSEUDO_PATH=fr)],
                            SC.CLASS_NAMES)
    assert only.pseudo_loader.fix_cp is None and only.pseudo_loader.pseudo_nms_thresh == 0.1
    aug.disable_augmentation(cfg)                                           # a fresh loader: the queue starts over
    assert aug.pseudo_loader is not loader


def test_deferred_copy_paste_after_world_op_raises(scenario):
    root, fr, st, frames = scenario
    cfg = SC.augmentor_config("no_gt_sampling", fr, st)
    ops = cfg['AUG_CONFIG_LIST']
    cfg['AUG_CONFIG_LIST'] = [ops[-4]] + ops[:-4]                           # a world op first
    aug = DA.DataAugmentor(Path(root), cfg, SC.CLASS_NAMES, deferred=True)
    with pytest.raises(ValueError):
        aug.forward(SC.data_dict(frames[0]))


def test_pickled_augmentor_continues_identically(scenario):
    np.random.seed(SC.seed_of("shipped"))
    aug = augmentor("shipped", scenario, deferred=True)
    frames = scenario[3]
    for frame in frames[:3]:
        aug.forward(SC.data_dict(frame))
    twin = pickle.loads(pickle.dumps(aug))
    assert queue_state(twin) == queue_state(aug)
    st = np.random.get_state()
    a = [aug.forward(SC.data_dict(f)) for f in frames[3:]]
    np.random.set_state(st)
    b = [twin.forward(SC.data_dict(f)) for f in frames[3:]]
    for x, y in zip(a, b):
        assert np.array_equal(x["points"], y["points"]) and np.array_equal(x["pseudo_boxes"], y["pseudo_boxes"])
    assert queue_state(twin) == queue_state(aug)


def test_stack_cut_boxes_forms():
    rng = np.random.default_rng(3)
    boxes = [syn.random_boxes(rng, 3), np.zeros((0, 7), np.float32), syn.random_boxes(rng, 2)]
    three = DA.stack_cut_boxes(boxes, [4, 0, 7])
    assert len(three) == 3 and three[0].shape == (5, 8) and three[1].tolist() == [0, 3, 3, 5] and three[2].tolist() == [4, 0, 7]
    four = DA.stack_cut_boxes(boxes, [4, 0, 7], [10, None, 7])
    assert len(four) == 4 and all(np.array_equal(x, y) for x, y in zip(three, four))
    assert four[3].dtype == np.int32 and four[3].tolist() == [10, DA.CUT_TO_END, 7]


@pytest.mark.parametrize("name", ["random_local_rotation", "random_local_scaling", "random_image_flip", "frustum_dropout_top",
                                  "imgaug"])
def test_other_ops_still_raise(name):
    with pytest.raises(NotImplementedError, match=name):
        DA.DataAugmentor(None, [SC.EDict(NAME=name)], SC.CLASS_NAMES)
