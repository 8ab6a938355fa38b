"""Raw scenes for the deferred augmentor on device-assembled sweeps (tests/test_raw_sweeps_augment.py,
tests/test_gpu_raw_sweeps_augment.py): the frames of pseudo_augment_scenario turned into scenes of
datasets.nuscenes_sweeps.pack_sweeps, and the two runs that the tests compare.

A frame's rows are dealt in order to a key frame and 3 to 5 sweeps; a sweep's rows go through the INVERSE of its rigid matrix
(sweeps_scenario.rigid), so that the host assembly (nuscenes_sweeps.assemble_host) brings them back to within rounding of where
they were and the unknown-class objects keep their points; one sweep has no matrix; ~2 % of a sweep's rows are replaced by ego
returns, which the assembly drops.  The host assembly of the raw scene is the yardstick scene: the host-mode augmentor runs on
it, the deferred augmentor on the raw scene itself."""
from pathlib import Path

import numpy as np

import pseudo_augment_scenario as SC
import sweeps_scenario as SW
from findnpropagate_amd.augmentor import data_augmentor as DA
from findnpropagate_amd.augmentor import database_sampler as DS
from findnpropagate_amd.datasets import nuscenes_sweeps as NS

PCR = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
RAW_SEED = 777          # of the split into sweeps; chosen with the case seeds of SC so that the host path alone meets the conditions


def raw_scene(points, index):
    """frame rows (N, 5) f32 -> a pack_sweeps scene [(raw (n, 5) f32, matrix or None, time_lag, is_key), ...]"""
    rng = np.random.default_rng(RAW_SEED + index)
    n_sweeps = 3 + index % 3
    cuts = np.sort(rng.integers(0, points.shape[0], n_sweeps))
    blocks = np.split(points, cuts)
    key = blocks[0].copy()
    key[:, 4] = rng.integers(0, 32, key.shape[0])
    scene = [(key, None, 0.0, True)]
    for j, blk in enumerate(blocks[1:], 1):
        matrix = None if j == 2 else SW.rigid(rng, j)
        raw = blk.copy()
        if matrix is not None:
            raw[:, :3] = ((blk[:, :3].astype(np.float64) - matrix[:3, 3]) @ matrix[:3, :3]).astype(np.float32)
        ego = rng.random(raw.shape[0]) < 0.02
        raw[ego, 0:2] = rng.uniform(-0.99, 0.99, (int(ego.sum()), 2))
        raw[:, 4] = rng.integers(0, 32, raw.shape[0])
        scene.append((np.ascontiguousarray(raw), matrix, 0.05 * j + 1e-3 * rng.random(), False))
    return scene


def raw_rows(scene):
    return sum(s[0].shape[0] for s in scene)


def host_dict(frame, scene):
    d = SC.data_dict(frame)
    d['points'] = NS.assemble_host(scene)
    return d


def raw_dict(frame, scene):
    d = SC.data_dict(frame)
    del d['points']
    d[DA.RAW_SWEEPS_KEY] = scene
    return d


def apply_world(points, d):
    """the four world ops of the host mode (data_augmentor.py, host branches, in queue order) with the parameters that a
    deferred run drew: flip x, flip y, rotation, scaling, translation"""
    p = np.asarray(points, np.float32).copy()
    if 'flip_x' not in d:
        return p
    if d['flip_x']:
        p[:, 1] = -p[:, 1]
    if d['flip_y']:
        p[:, 0] = -p[:, 0]
    p = DA.rotate_points_fused(p, d['noise_rot'])
    p[:, :3] *= d['noise_scale']
    p[:, :3] += d['noise_translate']
    return p


def final_rows_host(d, scene):
    """what the device chain makes of a deferred raw scene's data_dict, on the host: the lead rows, the assembled rows without
    those inside the cut boxes, the tail rows; then the programme's ops"""
    rows = NS.assemble_host(scene)
    boxes = d.get(DS.CUT_BOXES_KEY)
    if boxes is not None and len(boxes):
        rows = rows[DS.points_outside_boxes(rows, DS.cut_records(boxes))]
    lead = d.get(DA.LEAD_ROWS_KEY, np.zeros((0, 5), np.float32))
    tail = d.get(DA.TAIL_ROWS_KEY, np.zeros((0, 5), np.float32))
    return apply_world(np.concatenate([lead, rows, tail], 0), d)


class Recorder:
    """a scene-row provider that remembers the counts it answered"""

    def __init__(self, provider):
        self.provider, self.counts = provider, []

    def __call__(self, boxes7, cut_boxes=None):
        counts, rows = self.provider(boxes7, cut_boxes)
        self.counts.append(np.asarray(counts))
        return counts, rows


def queue_rows(aug):
    """the copy-paste queue as rows: per label and object (conf, box (8), num_points, points)"""
    out = []
    sampler = aug.pseudo_loader.sampler
    for label in sorted(sampler.unknown_queue):
        for o in sampler.unknown_queue[label]:
            out.append((label, float(o.conf), np.asarray(o.box), o.num_points, np.asarray(o.points),
                        (o.x, o.y, o.z, o.l, o.w, o.h, o.ry)))
    return out


def same_queue(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and x[1] == y[1] and np.array_equal(x[2], y[2]) and x[3] == y[3] and
                                    np.array_equal(x[4], y[4]) and x[5] == y[5] for x, y in zip(a, b))


def setup(tmp_path_factory):
    """-> (root, frustum folder, self-training folder, frames, raw scenes)"""
    root, fr, st = (str(tmp_path_factory.mktemp(n)) for n in ("db", "frustum", "selftrain"))
    SC.write_databases(root)
    frames = SC.make_frames(fr, st)
    return root, fr, st, frames, [raw_scene(f["points"], i) for i, f in enumerate(frames)]


def run_host(case, root, fr, st, frames, scenes):
    """the host-mode augmentor on the host assembly: per frame dict(points, gt_boxes, n_in: assembled rows, before / state:
    np.random's in front of and after the frame), and the queue after the last frame"""
    np.random.seed(SC.seed_of(case))
    aug = DA.DataAugmentor(Path(root), SC.augmentor_config(case, fr, st), SC.CLASS_NAMES)
    out = []
    for frame, scene in zip(frames, scenes):
        n_in = host_dict(frame, scene)['points'].shape[0]
        before = np.random.get_state()
        h = aug.forward(host_dict(frame, scene))
        out.append(dict(points=np.asarray(h['points'], np.float32), gt_boxes=h['gt_boxes'], n_in=n_in, before=before,
                        state=np.random.get_state()))
    return out, queue_rows(aug)


def run_deferred_points(case, root, fr, st, frames, scenes):
    """the deferred augmentor on the host assembly (the existing route): per frame its programme"""
    np.random.seed(SC.seed_of(case))
    aug = DA.DataAugmentor(Path(root), SC.augmentor_config(case, fr, st), SC.CLASS_NAMES, deferred=True)
    return [aug.forward(host_dict(frame, scene)).get(DA.PROGRAM_KEY) for frame, scene in zip(frames, scenes)]


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
