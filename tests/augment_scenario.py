"""Seeded scenario of the augmentation golden (tests/golden/make_augment_golden.py, tests/test_augmentor_golden.py): a few small
synthetic scenes with 9-column gt_boxes and pseudo_boxes, three augmentor configs (the config's order, another order, one op
disabled) and the mask + shuffle processor of transfusion_lidar.yaml.  Scene 3 of every case has no point inside the range."""
import numpy as np

POINT_CLOUD_RANGE = [-20.0, -20.0, -5.0, 20.0, 20.0, 3.0]
NUM_SCENES = 4
NUM_POINTS = 1800
CLASS_NAMES = ['car', 'truck', 'pedestrian']
CASES = ("config_order", "other_order", "rotation_disabled")
AUG_KEYS = ("points", "gt_boxes", "pseudo_boxes", "flip_x", "flip_y", "noise_rot", "noise_scale", "noise_translate")


class EDict(dict):
    """the attribute access of easydict.EasyDict, which the reference's configs are"""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


def _ops(case):
    flip = EDict(NAME='random_world_flip', ALONG_AXIS_LIST=['x', 'y'])
    rot = EDict(NAME='random_world_rotation', WORLD_ROT_ANGLE=[-0.78539816, 0.78539816])
    scale = EDict(NAME='random_world_scaling', WORLD_SCALE_RANGE=[0.9, 1.1])
    trans = EDict(NAME='random_world_translation', NOISE_TRANSLATE_STD=[0.5, 0.5, 0.5])
    if case == "other_order":
        return [trans, scale, rot, EDict(NAME='random_world_flip', ALONG_AXIS_LIST=['y', 'x'])]
    return [flip, rot, scale, trans]


def augmentor_config(case, wrap=EDict):
    """the list form for the first two cases, the AUG_CONFIG_LIST / DISABLE_AUG_LIST form for the third"""
    ops = _ops(case)
    if case == "rotation_disabled":
        gt = wrap(NAME='gt_sampling', USE_ROAD_PLANE=False)      # disabled too: never built
        return wrap(DISABLE_AUG_LIST=['gt_sampling', 'random_world_rotation'], AUG_CONFIG_LIST=[gt] + ops)
    return ops


def processor_config(wrap=EDict):
    return [wrap(NAME='mask_points_and_boxes_outside_range', REMOVE_OUTSIDE_BOXES=True),
            wrap(NAME='shuffle_points', SHUFFLE_ENABLED=wrap(train=True, test=True))]


def seed_of(case, s):
    return 1000 * (CASES.index(case) + 1) + s


def make_scene(case, s):
    """data_dict of scene s: points (NUM_POINTS, 5) over [-25, 25]^2 (some on the range's x / y ends), gt_boxes (8, 9),
    pseudo_boxes (5, 8).  Scene 3 lies wholly beyond x = 20 + 10."""
    rng = np.random.default_rng(seed_of(case, s))
    pts = np.empty((NUM_POINTS, 5), np.float32)
    pts[:, 0:2] = rng.uniform(-25, 25, (NUM_POINTS, 2))
    pts[:, 2] = rng.uniform(-3, 2, NUM_POINTS)
    pts[:, 3] = rng.uniform(0, 255, NUM_POINTS)
    pts[:, 4] = rng.choice(np.arange(10, dtype=np.float32) * 0.05, NUM_POINTS)
    pts[:8, 0] = [-20, 20, -20, 20, 5, -5, 20, -20]
    pts[8:16, 1] = [-20, 20, 20, -20, -20, 20, 3, -3]
    if s == 3:
        pts[:, 0] = np.abs(pts[:, 0]) + 30.0
    gt = np.zeros((8, 9), np.float32)
    gt[:, 0:2] = rng.uniform(-18, 18, (8, 2))
    gt[:, 2] = rng.uniform(-2, 0, 8)
    gt[:, 3:6] = rng.uniform(0.5, 5, (8, 3))
    gt[:, 6] = rng.uniform(-np.pi, np.pi, 8)
    gt[:, 7:9] = rng.normal(0, 3, (8, 2))
    gt[0, 0] = 24.0                              # a box outside the range (the mask drops it)
    pb = np.zeros((5, 8), np.float32)
    pb[:, 0:2] = rng.uniform(-18, 18, (5, 2))
    pb[:, 2] = rng.uniform(-2, 0, 5)
    pb[:, 3:6] = rng.uniform(0.5, 5, (5, 3))
    pb[:, 6] = rng.uniform(-np.pi, np.pi, 5)
    pb[:, 7] = rng.integers(1, 4, 5)
    return dict(points=pts, gt_boxes=gt, pseudo_boxes=pb, gt_names=np.array(CLASS_NAMES * 3)[:8])
