"""Seeded scenario of the gt_sampling golden (tests/golden/make_gt_sampling_golden.py, tests/test_gt_sampling_golden.py,
tests/test_gpu_gt_sampling.py): synthetic ground-truth databases (a dbinfos pickle plus one .bin file per object) written to a
directory, small scenes cut from synthetic.make_scene, and the sampler configs of the cases.

Every database holds the 10 nuScenes classes with 3-8 objects each (so the per-class pointers wrap within a few calls), 9-column
box3d_lidar, objects under the min-points filter and of difficulty -1.  The scenes carry float64 gt_boxes and gt_names with one
name outside CLASS_NAMES (gt_boxes_mask drops it)."""
import hashlib
import os
import pickle

import numpy as np

from findnpropagate_amd import synthetic as syn

CLASS_NAMES = ['car', 'truck', 'construction_vehicle', 'bus', 'trailer', 'barrier', 'motorcycle', 'bicycle', 'pedestrian',
               'traffic_cone']
SAMPLE_GROUPS = ['car:2', 'truck:3', 'construction_vehicle:7', 'bus:4', 'trailer:6', 'barrier:2', 'motorcycle:6', 'bicycle:6',
                 'pedestrian:2', 'traffic_cone:2']          # transfusion_lidar.yaml
SIZES = {'car': (4.6, 1.9, 1.7), 'truck': (7.0, 2.5, 3.0), 'construction_vehicle': (6.5, 2.8, 3.2), 'bus': (11.0, 2.9, 3.5),
         'trailer': (12.0, 2.9, 3.8), 'barrier': (0.5, 2.5, 1.0), 'motorcycle': (2.1, 0.8, 1.5), 'bicycle': (1.7, 0.6, 1.3),
         'pedestrian': (0.7, 0.7, 1.8), 'traffic_cone': (0.4, 0.4, 1.0)}
DATABASES = ("db5", "db6", "collide", "faces")
POINT_CLOUD_RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
WORLD_OPS = [dict(NAME='random_world_flip', ALONG_AXIS_LIST=['x', 'y']),
             dict(NAME='random_world_rotation', WORLD_ROT_ANGLE=[-0.78539816, 0.78539816]),
             dict(NAME='random_world_scaling', WORLD_SCALE_RANGE=[0.9, 1.1]),
             dict(NAME='random_world_translation', NOISE_TRANSLATE_STD=[0.5, 0.5, 0.5])]


class EDict(dict):
    """the attribute access of easydict.EasyDict, which the reference's configs are"""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


def _box(rng, name, centre_range=30.0):
    b = np.zeros(9, np.float64)
    b[0:2] = rng.uniform(-centre_range, centre_range, 2)
    size = np.array(SIZES[name]) * rng.uniform(0.85, 1.15, 3)
    b[3:6] = size
    b[2] = syn.GROUND_Z + size[2] / 2 + rng.uniform(-0.2, 0.2)
    b[6] = rng.uniform(-np.pi, np.pi)
    b[7:9] = rng.normal(0, 2, 2)
    return b


def _object_points(rng, box, n, cols):
    """n rows inside the box, relative to its centre (rotated with the box), intensity, and sweep times in the 6th column"""
    loc = rng.uniform(-0.5, 0.5, (n, 3)) * box[3:6]
    c, s = np.cos(box[6]), np.sin(box[6])
    p = np.zeros((n, cols), np.float32)
    p[:, 0] = loc[:, 0] * c - loc[:, 1] * s
    p[:, 1] = loc[:, 0] * s + loc[:, 1] * c
    p[:, 2] = loc[:, 2]
    p[:, 3] = rng.uniform(0, 255, n)
    p[:, 4] = rng.choice(np.arange(4, dtype=np.float32) * 0.05, n) if cols == 5 else 0.0
    if cols == 6:
        p[:, 5] = rng.choice(np.arange(10, dtype=np.float32) * 0.05, n)
    return p


def write_database(root, db):
    """Write database `db` under root: <db>_dbinfos.pkl and <db>_gt_database/*.bin.  Returns the SHA-256 of every file written."""
    rng = np.random.default_rng(DATABASES.index(db) + 77)
    cols = 6 if db == "db6" else 5
    sub = f"{db}_gt_database"
    os.makedirs(os.path.join(root, sub), exist_ok=True)
    infos = {c: [] for c in CLASS_NAMES}
    h = hashlib.sha256()
    for ci, name in enumerate(CLASS_NAMES):
        count = 1 if db == "faces" else int(rng.integers(3, 9))
        for k in range(count):
            box = _box(rng, name)
            if db == "collide" and k % 2 == 1:       # every other object sits on its predecessor: the sampled boxes collide
                box[0:2] = infos[name][-1]['box3d_lidar'][0:2] + rng.uniform(-0.3, 0.3, 2)
            if db == "faces":                         # headings 0 and pi/2 (tests/gt_sampling_scenario.face_points)
                box[6] = 0.0 if ci % 2 == 0 else np.pi / 2
                box[0:2] = [-30 + 6.0 * ci, 12.0 * (ci % 3) - 12.0]
            n = int(rng.integers(2, 30))
            pts = _object_points(rng, box, n, cols)
            rel = f"{sub}/{name}_{k}.bin"
            if k == 2:                                # one object per class stored as float64 (the reader's fallback)
                pts.astype(np.float64).tofile(os.path.join(root, rel))
            else:
                pts.tofile(os.path.join(root, rel))
            infos[name].append({'name': name, 'path': rel, 'image_idx': f"scene_{ci}_{k}", 'gt_idx': k, 'box3d_lidar': box,
                                'num_points_in_gt': n, 'difficulty': -1 if k == 1 else 0})
    with open(os.path.join(root, f"{db}_dbinfos.pkl"), "wb") as f:
        pickle.dump(infos, f, protocol=4)
    for rel in sorted([f"{db}_dbinfos.pkl"] + [os.path.join(sub, x) for x in os.listdir(os.path.join(root, sub))]):
        with open(os.path.join(root, rel), "rb") as f:
            h.update(rel.encode() + f.read())
    return h.hexdigest()


def sampler_config(case):
    """the gt_sampling entry of case `case` (the transfusion_lidar.yaml entry, varied)"""
    cfg = EDict(NAME='gt_sampling', DB_INFO_PATH=['db5_dbinfos.pkl'],
                PREPARE=EDict(filter_by_min_points=[f"{c}:5" for c in CLASS_NAMES]), SAMPLE_GROUPS=list(SAMPLE_GROUPS),
                NUM_POINT_FEATURES=5, DATABASE_WITH_FAKELIDAR=False, REMOVE_EXTRA_WIDTH=[0.0, 0.0, 0.0], LIMIT_WHOLE_SCENE=True)
    if case == "extra_width":
        cfg['REMOVE_EXTRA_WIDTH'] = [0.1, 0.3, 0.7]
    elif case == "sweeps_db":
        cfg.update(DB_INFO_PATH=['db6_dbinfos.pkl'], NUM_POINT_FEATURES=6)
    elif case == "time_range":
        cfg.update(DB_INFO_PATH=['db6_dbinfos.pkl'], NUM_POINT_FEATURES=6, FILTER_OBJ_POINTS_BY_TIMESTAMP=True,
                   TIME_RANGE=[0.3, 0.0])
    elif case == "collide":
        cfg.update(DB_INFO_PATH=['collide_dbinfos.pkl'], LIMIT_WHOLE_SCENE=False)
    elif case == "prepare":
        cfg['PREPARE'] = EDict(filter_by_min_points=['car:12', 'truck:0', 'bus:20', 'nothing:3'], filter_by_difficulty=[-1])
    elif case == "faces":
        cfg.update(DB_INFO_PATH=['faces_dbinfos.pkl'], SAMPLE_GROUPS=['car:1', 'truck:1', 'bus:1', 'barrier:1'],
                   PREPARE=EDict(filter_by_min_points=[]))
    return cfg


# case -> (calls, world ops after gt_sampling?)
CASES = {"transfusion": (6, True), "no_gt": (2, False), "limit_scene": (1, False), "extra_width": (2, True),
         "sweeps_db": (1, False), "time_range": (1, False), "collide": (2, False), "prepare": (2, False), "faces": (1, True)}


def augmentor_config(case):
    return [sampler_config(case)] + ([EDict(o) for o in WORLD_OPS] if CASES[case][1] else [])


def seed_of(case):
    return 4000 + list(CASES).index(case)


def face_points(boxes):
    """rows on the faces of the (M, 7) boxes: local x or y at +-1 ulp around d/2 + 1e-2 and exactly there, z at +-dz/2"""
    rows = []
    for b in boxes:
        c, s = np.cos(b[6]), np.sin(b[6])
        for ax in (0, 1):
            e = np.float32(b[3 + ax] / 2 + 1e-2)
            for v in (np.nextafter(e, np.float32(0)), e, np.nextafter(e, np.float32(9)), np.float32(b[3 + ax] / 2)):
                for sign in (1, -1):
                    lx, ly = (sign * v, 0.0) if ax == 0 else (0.0, sign * v)
                    rows.append([b[0] + lx * c - ly * s, b[1] + lx * s + ly * c, b[2]])
        for dz in (b[5] / 2, -b[5] / 2):
            rows.append([b[0], b[1], b[2] + dz])
            rows.append([b[0], b[1], np.nextafter(np.float32(b[2] + dz), np.float32(0))])
    return np.asarray(rows, np.float32)


def make_scene(case, call):
    """data_dict of one call: ~1200 points of a synthetic sweep, float64 gt_boxes (9 columns), gt_names, gt_boxes_mask"""
    seed = seed_of(case) * 10 + call
    rng = np.random.default_rng(seed)
    pts = syn.make_scene(seed)[::25].copy()
    n_gt = 0 if case == "no_gt" else 6
    gt = np.zeros((n_gt, 9), np.float64)
    names = []
    for k in range(n_gt):
        name = 'car' if (case == "limit_scene" and k < 4) else CLASS_NAMES[int(rng.integers(0, 10))]
        gt[k] = _box(rng, name, centre_range=45.0)
        names.append(name)
    if n_gt:
        names[-1] = 'ignore'                          # not in CLASS_NAMES: gt_boxes_mask drops it
    names = np.array(names) if names else np.zeros((0,), '<U10')
    d = dict(points=pts, gt_boxes=gt, gt_names=names,
             gt_boxes_mask=np.array([n in CLASS_NAMES for n in names], dtype=np.bool_))
    return d


def add_face_points(d, db_root):
    """the faces case: rows on the faces of every box of the faces database, appended to the scene"""
    with open(os.path.join(db_root, "faces_dbinfos.pkl"), "rb") as f:
        infos = pickle.load(f)
    boxes = np.stack([infos[c][0]['box3d_lidar'][:7] for c in ('car', 'truck', 'bus', 'barrier')]).astype(np.float32)
    fp = face_points(boxes)
    rows = np.zeros((fp.shape[0], d['points'].shape[1]), np.float32)
    rows[:, :3] = fp
    rows[:, 3] = 7.0
    d['points'] = np.concatenate([d['points'], rows], 0)
    return d
