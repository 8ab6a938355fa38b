"""gt_sampling (DataBaseSampler + DataAugmentor.gt_sampling) against the reference's own DataAugmentor and DataBaseSampler
(tests/golden/gt_sampling_golden.npz, made by tests/golden/make_gt_sampling_golden.py), bit for bit: points, gt_boxes, gt_names
and the np.random draw that comes next, call after call of one sampler.  The deferred mode draws the same, puts the object rows
in front of the untested scene rows and records the cut.  The host cut against the reference's points_in_boxes_cpu masks.
CPU only."""
import logging
import os
import pickle
from pathlib import Path

import numpy as np
import pytest
import torch

import gt_sampling_scenario as SC
from findnpropagate_amd import synthetic as syn
from findnpropagate_amd.augmentor import data_augmentor as DA
from findnpropagate_amd.augmentor import database_sampler as DS
from test_oracle_ops import pib_inputs_sha256, pib_trials

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gt_sampling_golden.npz")
PIB_GOLD = os.path.join(HERE, "golden", "pib_cpu_ref.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def db_root(tmp_path_factory, golden):
    root = tmp_path_factory.mktemp("gt_database")
    for db in SC.DATABASES:
        assert SC.write_database(str(root), db) == str(golden[f"db_sha256/{db}"]), f"database {db} drifted from the golden's"
    return root


def scene(case, call, root):
    d = SC.make_scene(case, call)
    return SC.add_face_points(d, str(root)) if case == "faces" else d


def next_draw():
    st = np.random.get_state()
    v = np.random.random()
    np.random.set_state(st)
    return v


def run_case(case, root, deferred=False, sampler_only=False):
    """every call of the case through one augmentor (or one sampler): [(input scene, output, next draw)]"""
    np.random.seed(SC.seed_of(case))
    if sampler_only:
        fn = DS.DataBaseSampler(Path(root), SC.sampler_config(case), SC.CLASS_NAMES, deferred=deferred)
    else:
        fn = DA.DataAugmentor(Path(root), SC.augmentor_config(case), SC.CLASS_NAMES, deferred=deferred).forward
    res = []
    for call in range(SC.CASES[case][0]):
        d = scene(case, call, root)
        raw = {k: v.copy() for k, v in d.items()}
        out = fn(d)
        res.append((raw, out, next_draw()))
    return res


def check(golden, key, out, draw):
    for k in ("points", "gt_boxes"):
        got, exp = np.asarray(out[k]), golden[f"{key}/{k}"]
        assert got.dtype == exp.dtype and got.shape == exp.shape, (key, k, got.dtype, exp.dtype, got.shape, exp.shape)
        assert np.array_equal(got, exp), (key, k)
    assert np.array_equal(np.asarray(out["gt_names"]).astype(str), golden[f"{key}/gt_names"]), key
    assert draw == golden[f"{key}/next_draw"], key


@pytest.mark.parametrize("case", list(SC.CASES))
def test_host_augmentor_matches_reference(golden, db_root, case):
    for call, (_, out, draw) in enumerate(run_case(case, db_root)):
        check(golden, f"{case}/{call}", out, draw)


def test_golden_exercises_the_cases(golden):
    """the fixture cuts scene points, pastes objects, wraps pointers and leaves some calls without gt boxes"""
    n_in = {c: SC.make_scene(c, 0)["points"].shape[0] for c in SC.CASES}
    assert golden["no_gt/0/gt_boxes"].shape[0] > 0                      # sampled into a scene without gt boxes
    sp = golden["sampler/transfusion/0/points"]
    assert sp.shape[0] != n_in["transfusion"]
    assert golden["collide/0/gt_boxes"].shape[0] < 5 + sum(int(g.split(':')[1]) for g in SC.SAMPLE_GROUPS)


@pytest.mark.parametrize("case", [c for c in ("transfusion", "no_gt", "extra_width", "faces")])
def test_host_sampler_matches_reference(golden, db_root, case):
    for call, (_, out, draw) in enumerate(run_case(case, db_root, sampler_only=True)):
        check(golden, f"sampler/{case}/{call}", out, draw)
        assert "gt_boxes_mask" not in out


@pytest.mark.parametrize("case", list(SC.CASES))
def test_deferred_sampler_records_the_cut(golden, db_root, case):
    """deferred: the same boxes, names and draws; points = object rows + every scene row; the recorded cut, applied on the host,
    gives the host mode's points"""
    host = run_case(case, db_root, sampler_only=True)
    dfr = run_case(case, db_root, deferred=True, sampler_only=True)
    for (raw, h, hd), (_, d, dd) in zip(host, dfr):
        assert hd == dd
        assert np.array_equal(h["gt_boxes"], d["gt_boxes"]) and np.array_equal(h["gt_names"], d["gt_names"])
        boxes, cut_from = d[DS.CUT_BOXES_KEY], d[DS.CUT_FROM_KEY]
        assert boxes.dtype == np.float32 and boxes.shape[1] == 7 and isinstance(cut_from, int)
        n_raw = raw["points"].shape[0]
        assert d["points"].shape[0] == cut_from + n_raw
        assert np.array_equal(d["points"][cut_from:], raw["points"])
        keep = DS.points_outside_boxes(d["points"][cut_from:, :3], DS.cut_records(boxes))
        want = np.concatenate([d["points"][:cut_from], raw["points"][keep]])
        assert want.dtype == h["points"].dtype and np.array_equal(want, h["points"])
        assert np.array_equal(d["points"][:cut_from], h["points"][:cut_from])


@pytest.mark.parametrize("case", ["transfusion", "extra_width", "faces"])
def test_deferred_augmentor_draws_the_same(golden, db_root, case):
    for call, (_, out, draw) in enumerate(run_case(case, db_root, deferred=True)):
        key = f"{case}/{call}"
        assert np.array_equal(out["gt_boxes"], golden[f"{key}/gt_boxes"])
        assert np.array_equal(out["gt_names"].astype(str), golden[f"{key}/gt_names"])
        assert draw == golden[f"{key}/next_draw"]
        assert DA.PROGRAM_KEY in out and DS.CUT_BOXES_KEY in out


def test_enlarge_rounds_like_the_reference():
    """check_numpy_to_torch casts the boxes to f32 before enlarge_box3d adds the width in f32"""
    b = np.array([[1.0, 2.0, 0.5, 4.123456789, 1.987654321, 1.5, 0.3]], np.float64)
    t = torch.from_numpy(b).float()
    t[:, 3:6] += t.new_tensor([0.1, 0.3, 0.7])[None, :]
    assert np.array_equal(DS.enlarge_cut_boxes(b, [0.1, 0.3, 0.7]), t.numpy())


def test_host_cut_matches_reference_points_in_boxes_cpu(rng):
    """fnp_host_points_outside_boxes = not(column-OR) of the reference's masks (tests/golden/pib_cpu_ref.npz)"""
    gold = np.load(PIB_GOLD)
    for trial, (boxes, pts) in enumerate(pib_trials(rng)):
        assert pib_inputs_sha256(boxes, pts) == str(gold[f"inputs_sha256_{trial}"])
        shape = (boxes.shape[0], pts.shape[0])
        want = np.unpackbits(gold[f"mask_{trial}"], count=shape[0] * shape[1]).reshape(shape)
        keep = DS.points_outside_boxes(pts, DS.cut_records(boxes))
        assert np.array_equal(keep, want.sum(0) == 0)
        assert (~keep).sum() > 0
        for b in range(boxes.shape[0]):        # box by box: each mask row
            assert np.array_equal(~DS.points_outside_boxes(pts, DS.cut_records(boxes[b:b + 1])), want[b] == 1)


def test_host_cut_with_wider_rows_and_no_boxes():
    rng = np.random.default_rng(3)
    pts = rng.uniform(-5, 5, (3000, 6)).astype(np.float32)
    boxes = syn.random_boxes(rng, 9, centre_range=4.0)
    rec = DS.cut_records(boxes)
    assert np.array_equal(DS.points_outside_boxes(pts, rec), DS.points_outside_boxes(np.ascontiguousarray(pts[:, :3]), rec))
    assert DS.points_outside_boxes(pts, rec[:0]).all()
    assert DS.points_outside_boxes(pts[:0], rec).shape == (0,)
    assert np.array_equal(rec[:, :6], boxes[:, :6])
    assert np.abs(rec[:, 6] - np.cos(-boxes[:, 6].astype(np.float64))).max() < 1e-6
    assert np.abs(rec[:, 7] - np.sin(-boxes[:, 6].astype(np.float64))).max() < 1e-6


def test_stack_cut_boxes():
    a = np.arange(14, dtype=np.float32).reshape(2, 7)
    b = np.zeros((0, 7), np.float32)
    c = np.ones((3, 7), np.float32)
    rec, off, cf = DA.stack_cut_boxes([a, b, c], [5, 0, 7])
    assert rec.shape == (5, 8) and rec.dtype == np.float32
    assert off.dtype == np.int32 and off.tolist() == [0, 2, 2, 5]
    assert cf.dtype == np.int32 and cf.tolist() == [5, 0, 7]
    assert np.array_equal(rec, DS.cut_records(np.concatenate([a, c])))
    rec, off, cf = DA.stack_cut_boxes([b], [0])
    assert rec.shape == (0, 8) and off.tolist() == [0, 0]


def test_unsupported_keys_name_themselves(db_root):
    base = SC.sampler_config("transfusion")
    for key, val in (("USE_ROAD_PLANE", True), ("IMG_AUG_TYPE", "kitti"), ("USE_SHARED_MEMORY", True),
                     ("DATABASE_WITH_FAKELIDAR", True)):
        cfg = SC.EDict(base, **{key: val})
        with pytest.raises(NotImplementedError, match=key):
            DA.DataAugmentor(Path(db_root), [cfg], SC.CLASS_NAMES)
    cfg = SC.EDict(base, DB_INFO_PATH=["missing.pkl"], BACKUP_DB_INFO=dict(DB_INFO_PATH="x.pkl", DB_DATA_PATH=["y.npy"]))
    with pytest.raises(NotImplementedError, match="BACKUP_DB_INFO"):
        DA.DataAugmentor(Path(db_root), [cfg], SC.CLASS_NAMES)
    with pytest.raises(NotImplementedError, match="gt_sampling"):
        DA.DataAugmentor(None, [base], SC.CLASS_NAMES)
    assert len(DA.DataAugmentor(Path(db_root), [SC.EDict(base, USE_ROAD_PLANE=False)], SC.CLASS_NAMES).data_augmentor_queue) == 1


def test_deferred_gt_sampling_after_a_world_op_is_refused(db_root):
    ops = [SC.EDict(o) for o in SC.WORLD_OPS[:1]] + [SC.sampler_config("transfusion")]
    np.random.seed(0)
    aug = DA.DataAugmentor(Path(db_root), ops, SC.CLASS_NAMES, deferred=True)
    with pytest.raises(ValueError):
        aug.forward(SC.make_scene("transfusion", 0))
    host = DA.DataAugmentor(Path(db_root), ops, SC.CLASS_NAMES)   # host mode cuts the moved points: allowed
    host.forward(SC.make_scene("transfusion", 0))


def test_sampler_pickles_with_its_state(db_root):
    np.random.seed(SC.seed_of("transfusion"))
    s = DS.DataBaseSampler(Path(db_root), SC.sampler_config("transfusion"), SC.CLASS_NAMES, logger=logging.getLogger("gt_sampling_test"))
    s(SC.make_scene("transfusion", 0))
    t = pickle.loads(pickle.dumps(s))
    assert not hasattr(t, "logger")
    for name, g in s.sample_groups.items():
        assert t.sample_groups[name]['pointer'] == g['pointer'] and np.array_equal(t.sample_groups[name]['indices'], g['indices'])
    st = np.random.get_state()
    a = s(SC.make_scene("transfusion", 1))
    np.random.set_state(st)
    b = t(SC.make_scene("transfusion", 1))
    assert np.array_equal(a["points"], b["points"]) and np.array_equal(a["gt_boxes"], b["gt_boxes"])
    aug = DA.DataAugmentor(Path(db_root), SC.augmentor_config("transfusion"), SC.CLASS_NAMES)
    assert len(pickle.loads(pickle.dumps(aug)).data_augmentor_queue) == 5
