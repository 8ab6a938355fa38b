"""sparse.prepare_points with the 4-tuple cut (fnp_prepare_points_cut_window): gt_sampling's cut bounded by the prep_cut_to that a
deferred unknowns_copy_paste records, so that the pasted rows behind the scene rows are never cut.

The deferred augmentor of the self-training queue, the deferred processor and prepare_points with the caller's numpy
permutation are compared bit for bit with the host path (host-mode DataAugmentor, mask, np.random.permutation) on the fixture
sequences; the window alone with the host cut on edge cases and ten-sweep-sized scenes; the voxeliser with the oracle; the
3-tuple path with the window "to the end"; and a captured graph replayed with other records and other windows."""
from pathlib import Path

import numpy as np
import pytest
import torch

import augment_scenario as AS
import pseudo_augment_scenario as SC
from findnpropagate_amd import sparse as S
from findnpropagate_amd import synthetic as syn
from findnpropagate_amd.augmentor import data_augmentor as DA
from findnpropagate_amd.augmentor import database_sampler as DS
from findnpropagate_amd.processor.data_processor import DataProcessor
from test_gpu_gt_sampling import BIG, WORLD, sampled_boxes
from test_gpu_prepare_points import SMALL_RANGE, _voxelize_check, check_prepared, host_prepare, to_dev

pytestmark = pytest.mark.gpu

PCR = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]


def cut4_to_dev(boxes_list, cut_from_list, cut_to_list, dev):
    return tuple(torch.from_numpy(a).to(dev) for a in DA.stack_cut_boxes(boxes_list, cut_from_list, cut_to_list))


def host_window(scene, records, lo, hi):
    keep = np.ones(scene.shape[0], bool)
    keep[lo:hi] = DS.points_outside_boxes(scene[lo:hi], records)
    return scene[keep]


def _processor(deferred):
    return DataProcessor(AS.processor_config(), np.array(PCR, np.float32), training=True, num_point_features=5, deferred=deferred)


@pytest.fixture(scope="module")
def sequences(tmp_path_factory):
    """per case and frame: the host path (final points, drawn permutation) and the deferred data_dict"""
    root, fr, st = (str(tmp_path_factory.mktemp(n)) for n in ("db", "frustum", "selftrain"))
    SC.write_databases(root)
    frames = SC.make_frames(fr, st)
    res = []
    for case in SC.CASES:
        np.random.seed(SC.seed_of(case))
        cfg = SC.augmentor_config(case, fr, st)
        host_aug = DA.DataAugmentor(Path(root), cfg, SC.CLASS_NAMES)
        dfr_aug = DA.DataAugmentor(Path(root), cfg, SC.CLASS_NAMES, deferred=True)
        for frame in frames:
            st_ = np.random.get_state()
            h = host_aug.forward(SC.data_dict(frame))
            after = np.random.get_state()
            drawn = []
            perm_fn = np.random.permutation
            try:
                np.random.permutation = lambda n: drawn.append(perm_fn(n)) or drawn[-1]
                h = _processor(False).forward(h)
            finally:
                np.random.permutation = perm_fn
            np.random.set_state(st_)
            d = _processor(True).forward(dfr_aug.forward(SC.data_dict(frame)))
            assert np.random.get_state()[2] == after[2] and np.array_equal(np.random.get_state()[1], after[1])
            res.append(dict(case=case, final=np.asarray(h["points"], np.float32), perm=drawn[0].astype(np.int32), d=d))
    return res


def test_fixture_sequences_match_host(cuda, sequences):
    scenes = [np.asarray(c["d"]["points"], np.float32) for c in sequences]
    programs = [c["d"].get(DA.PROGRAM_KEY, np.zeros((0, 4), np.float32)) for c in sequences]
    pts, off, prog = to_dev(scenes, programs, cuda)
    cut = cut4_to_dev([c["d"].get(DS.CUT_BOXES_KEY, np.zeros((0, 7), np.float32)) for c in sequences],
                      [c["d"].get(DS.CUT_FROM_KEY, 0) for c in sequences], [c["d"].get(DA.CUT_TO_KEY) for c in sequences], cuda)
    assert int(cut[1][-1].item()) > 0 and any(DA.CUT_TO_KEY in c["d"] for c in sequences)
    perm = torch.from_numpy(np.concatenate([c["perm"] for c in sequences])).to(cuda)
    res = S.prepare_points(pts, off, len(sequences), prog, PCR, shuffle=perm, cut=cut)
    check_prepared(res, [c["final"] for c in sequences], pts.shape[0])


def window_cases(rng):
    def scene(n, lo=-20, hi=20):
        p = rng.uniform(lo, hi, (n, 5)).astype(np.float32)
        p[:, 2] = rng.uniform(-3, 2, n)
        return p
    base = scene(3000)
    bx = syn.random_boxes(rng, 12, centre_range=15.0)
    inside = scene(400, -1, 1)
    one = np.array([[0, 0, 0, 4, 4, 8, 0.3]], np.float32)
    return [  # (scene, boxes, cut_from, cut_to)
        (base, bx, 100, 100),                              # cut_to == cut_from: nothing is cut
        (base, bx, 100, 3000),                             # cut_to == the scene length
        (base, bx, 50, 10 ** 6),                           # past the scene length
        (base, bx, 0, None),                               # to the end
        (np.concatenate([scene(200), inside]), one, 0, 200),   # pasted rows inside the cut box are kept
        (scene(500), np.zeros((0, 7), np.float32), 0, 300),    # no records
        (scene(0), bx, 0, 0),
        (base, bx, 700, 2100),
    ]


def test_window_edge_cases(cuda):
    rng = np.random.default_rng(31)
    cases = window_cases(rng)
    for batch in (cases, cases[4:5], cases[1:4]):
        finals = [host_window(s, DS.cut_records(b), lo, DA.CUT_TO_END if hi is None else hi) for s, b, lo, hi in batch]
        p, off, _ = to_dev([c[0] for c in batch], [], cuda)
        res = S.prepare_points(p, off, len(batch), None, BIG, cut=cut4_to_dev(*zip(*[(c[1], c[2], c[3]) for c in batch]), cuda))
        check_prepared(res, finals, p.shape[0])
    kept = host_window(cases[4][0], DS.cut_records(cases[4][1]), 0, 200)
    assert np.array_equal(kept[-400:], cases[4][0][-400:])
    assert not DS.points_outside_boxes(cases[4][0][-400:], DS.cut_records(cases[4][1])).any()   # a full cut drops them


def test_three_tuple_equals_window_to_the_end(cuda):
    rng = np.random.default_rng(32)
    pts, o = syn.make_batch([4, 5, 6])
    scenes = [pts[o[b]:o[b + 1]] for b in range(3)]
    boxes = [sampled_boxes(rng, k, s) for k, s in zip((12, 0, 20), scenes)]
    _, programs, _ = host_prepare(scenes, [7, 8, 9], WORLD, syn.POINT_CLOUD_RANGE)
    p, off, prog = to_dev(scenes, programs, cuda)
    three = tuple(torch.from_numpy(a).to(cuda) for a in DA.stack_cut_boxes(boxes, [30, 0, 5]))
    a = S.prepare_points(p, off, 3, prog, syn.POINT_CLOUD_RANGE, shuffle="device", seed=5, cut=three)
    a = (a["points"].clone(), a["batch_offsets"].clone())
    b = S.prepare_points(p, off, 3, prog, syn.POINT_CLOUD_RANGE, shuffle="device", seed=5,
                         cut=cut4_to_dev(boxes, [30, 0, 5], [None, None, None], cuda))
    assert torch.equal(a[0], b["points"]) and torch.equal(a[1], b["batch_offsets"])


def test_ten_sweep_scenes_with_pasted_rows(cuda):
    """4 ten-sweep scenes (~300 k points): 2000 leading object rows, the scene, 1500 pasted rows inside the cut boxes"""
    pts, o = syn.make_sweeps_batch([0, 1, 2, 3])
    rng = np.random.default_rng(33)
    scenes, boxes, lo, hi, cut_scenes = [], [], [], [], []
    for b in range(4):
        sc = pts[o[b]:o[b + 1]]
        obj = sc[rng.integers(0, sc.shape[0], 2000)]
        bx = sampled_boxes(rng, 39, sc)
        n_scene = obj.shape[0] + sc.shape[0]
        pasted = np.repeat(bx[:, None, :3], 40, 1).reshape(-1, 3)
        pasted = np.concatenate([pasted, rng.uniform(0, 1, (pasted.shape[0], 2))], 1).astype(np.float32)
        full = np.concatenate([obj, sc, pasted])
        scenes.append(full)
        boxes.append(bx)
        lo.append(obj.shape[0])
        hi.append(n_scene)
        cut_scenes.append(host_window(full, DS.cut_records(bx), obj.shape[0], n_scene))
    assert all(c[-1560:].shape[0] == 1560 and np.array_equal(c[-1560:], s[-1560:]) for c, s in zip(cut_scenes, scenes))
    finals, programs, perms = host_prepare(cut_scenes, [51, 52, 53, 54], WORLD, syn.POINT_CLOUD_RANGE)
    p, off, prog = to_dev(scenes, programs, cuda)
    res = S.prepare_points(p, off, 4, prog, syn.POINT_CLOUD_RANGE, shuffle=torch.from_numpy(np.concatenate(perms)).to(cuda),
                           cut=cut4_to_dev(boxes, lo, hi, cuda))
    check_prepared(res, finals, p.shape[0])


def test_voxelize_windowed_batch_matches_oracle(cuda, oracle):
    pts, o = syn.make_sweeps_batch([5, 6])
    rng = np.random.default_rng(34)
    scenes, boxes, cut_scenes, his = [], [], [], []
    for b in range(2):
        sc = pts[o[b]:o[b + 1]]
        bx = sampled_boxes(rng, 39, sc[np.abs(sc[:, 0]).clip(0, 99) < 12])
        hi = sc.shape[0] - 5000
        scenes.append(sc)
        boxes.append(bx)
        his.append(hi)
        cut_scenes.append(host_window(sc, DS.cut_records(bx), 0, hi))
    finals, programs, perms = host_prepare(cut_scenes, [71, 72], WORLD, SMALL_RANGE)
    p, off, prog = to_dev(scenes, programs, cuda)
    res = S.prepare_points(p, off, 2, prog, SMALL_RANGE, shuffle=torch.from_numpy(np.concatenate(perms)).to(cuda),
                           cut=cut4_to_dev(boxes, [0, 0], his, cuda))
    check_prepared(res, finals, p.shape[0])
    assert _voxelize_check(oracle, res, finals, SMALL_RANGE, 160000) > 10000


def test_window_captures_and_replays(cuda):
    pts, o = syn.make_batch([0, 1, 2])
    scenes = [pts[o[b]:o[b + 1]] for b in range(3)]
    rng = np.random.default_rng(35)
    sets = []
    for _ in range(2):
        bx = [sampled_boxes(rng, k, s) for k, s in zip((10, 0, 14), scenes)]
        lo = [int(rng.integers(0, 500)) for _ in scenes]
        sets.append((bx, lo, [int(l + rng.integers(0, s.shape[0])) for l, s in zip(lo, scenes)]))
    _, programs, _ = host_prepare(scenes, [1, 2, 3], WORLD, syn.POINT_CLOUD_RANGE)
    p, off, prog = to_dev(scenes, programs, cuda)
    eager = []
    for s in sets:
        r = S.prepare_points(p, off, 3, prog, syn.POINT_CLOUD_RANGE, shuffle="device", seed=3, cut=cut4_to_dev(*s, cuda))
        eager.append((r["points"].clone(), r["batch_offsets"].clone()))
    assert not torch.equal(eager[0][1], eager[1][1])
    static = cut4_to_dev(*sets[0], cuda)
    out = S.prepare_points(p, off, 3, prog, syn.POINT_CLOUD_RANGE, shuffle="device", seed=3, cut=static)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            S.prepare_points(p, off, 3, prog, syn.POINT_CLOUD_RANGE, shuffle="device", seed=3, cut=static, out=out)
    torch.cuda.current_stream().wait_stream(s)
    for k in (1, 0):
        for t, new in zip(static, cut4_to_dev(*sets[k], cuda)):
            t.copy_(new)
        out["points"].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["points"], eager[k][0]) and torch.equal(out["batch_offsets"], eager[k][1])
