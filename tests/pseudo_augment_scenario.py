"""Seeded inputs of the pseudo-label augmentor golden (tests/golden/make_pseudo_augment_golden.py, which runs the REFERENCE's
DataAugmentor on them, tests/test_pseudo_augment_golden.py and tests/test_gpu_pseudo_augment.py): the augmentor queue of the
shipped self-training configuration (gt_sampling, load_frustum_pseudos, load_selftrain_pseudos, unknowns_copy_paste, the four
world ops) over sequences of frames, because the copy-paste queue carries state from frame to frame.

The frames and their frustum / self-training .pth files are those of tests/pseudo_scenario.py, thinned to every 32nd row plus
every row near an unknown-class object (those objects keep their points, so the queue fills).  The databases are gt_sampling_scenario's
db5 and "near": known-class objects placed against the unknown-class objects of the frames, so that sampled boxes overlap
copy boxes and pasted objects (the `overlap` case)."""
import os
import pickle

import numpy as np

import gt_sampling_scenario as GS
import pseudo_scenario as PS
from findnpropagate_amd import synthetic as syn

KNOWN = PS.KNOWN
CLASS_NAMES = list(KNOWN)          # the shipped configuration trains the 6 known classes
N_FRAMES = PS.N_FRAMES
EDict = GS.EDict


def _scene_boxes(i):
    _, boxes, cls = syn.make_scene(200 + i, n_azimuth=400, n_boxes=24, return_boxes=True)
    return boxes, [PS.ALL[c] for c in cls]


def _near_any(points, boxes, pad=0.3):
    """rows within `pad` of one of the boxes (f64 box-frame test; only thins the scene)"""
    near = np.zeros(points.shape[0], bool)
    for b in boxes:
        d = points[:, :2].astype(np.float64) - b[:2]
        c, s = np.cos(-b[6]), np.sin(-b[6])
        lx, ly = d[:, 0] * c - d[:, 1] * s, d[:, 0] * s + d[:, 1] * c
        near |= (np.abs(lx) <= b[3] / 2 + pad) & (np.abs(ly) <= b[4] / 2 + pad)
    return near


def make_frames(folder_frustum, folder_st):
    """-> per-frame data_dict makers' inputs: frame_id, points (N, 5) f32, gt_boxes (G, 9) f64, gt_names; writes the .pth files"""
    frames = []
    for i, fr in enumerate(PS.make_frames(folder_frustum, folder_st)):
        pts = fr["points"]
        boxes, names = _scene_boxes(i)
        keep = _near_any(pts, boxes[[n not in KNOWN for n in names]])
        keep[::32] = True
        g = fr["gt_boxes"]
        gt = np.zeros((g.shape[0], 9), np.float64)
        gt[:, :7] = g[:, :7]
        gt[:, 7:9] = np.round(np.sin(np.arange(2 * g.shape[0]).reshape(-1, 2) + i), 3)
        names = np.array([KNOWN[int(l) - 1] for l in g[:, 7]])
        frames.append(dict(frame_id=fr["frame_id"], points=np.ascontiguousarray(pts[keep]), gt_boxes=gt, gt_names=names))
    return frames


def data_dict(frame):
    return dict(frame_id=frame["frame_id"], points=frame["points"].copy(), gt_boxes=frame["gt_boxes"].copy(),
                gt_names=frame["gt_names"].copy(), gt_boxes_mask=np.ones(frame["gt_boxes"].shape[0], np.bool_))


def write_near_database(root):
    """near_dbinfos.pkl: per known class 5 objects, each against an unknown-class object of one frame (shifted by ~0.8 of the
    two half lengths along the object's heading, so that the boxes overlap a little).  Returns the SHA-256 of the files."""
    import hashlib
    rng = np.random.default_rng(123)
    sub = "near_gt_database"
    os.makedirs(os.path.join(root, sub), exist_ok=True)
    unknown = []
    for i in range(N_FRAMES):
        boxes, names = _scene_boxes(i)
        unknown += [b for b, n in zip(boxes, names) if n not in KNOWN]
    infos = {c: [] for c in GS.CLASS_NAMES}
    h = hashlib.sha256()
    j = 0
    for name in GS.CLASS_NAMES:
        for k in range(5):
            u = unknown[(j * 7) % len(unknown)]
            j += 1
            box = np.zeros(9, np.float64)
            box[3:6] = np.array(GS.SIZES[name]) * rng.uniform(0.9, 1.1, 3)
            shift = 0.8 * (u[3] / 2 + box[3] / 2)
            box[0:2] = u[0:2] + shift * np.array([np.cos(u[6]), np.sin(u[6])])
            box[2] = syn.GROUND_Z + box[5] / 2
            box[6] = u[6] + rng.uniform(-0.2, 0.2)
            n = int(rng.integers(8, 30))
            pts = GS._object_points(rng, box, n, 5)
            rel = f"{sub}/{name}_{k}.bin"
            pts.tofile(os.path.join(root, rel))
            infos[name].append({'name': name, 'path': rel, 'image_idx': f"near_{j}", 'gt_idx': k, 'box3d_lidar': box,
                                'num_points_in_gt': n, 'difficulty': 0})
    with open(os.path.join(root, "near_dbinfos.pkl"), "wb") as f:
        pickle.dump(infos, f, protocol=4)
    for rel in sorted(["near_dbinfos.pkl"] + [os.path.join(sub, x) for x in os.listdir(os.path.join(root, sub))]):
        with open(os.path.join(root, rel), "rb") as f:
            h.update(rel.encode() + f.read())
    return h.hexdigest()


def write_databases(root):
    """-> {db: sha256} of db5 and near under root"""
    return {"db5": GS.write_database(root, "db5"), "near": write_near_database(root)}


SHIPPED_LOADER = dict(DROPOUT=0.2, MIN_SCORE=0.1, PSEUDO_NMS_THRESH=0.1, FIX_CP=10, MOMENTUM=0.9997, COPY_ST_ONLY=True,
                      SAMPLER_VAL=False)
SHIPPED_QUEUE = dict(MAX_QUEUE_SIZE=60, QUEUE_METRIC='conf', TRANS_NOISE=1.0, ROT_NOISE=0.785)

# case -> (database or None for no gt_sampling, loader keys over the shipped ones, queue keys over the shipped ones, world ops?)
CASES = {
    "shipped": ("db5", {}, {}, True),
    "num_pts": ("db5", {}, dict(QUEUE_METRIC='num_pts', MAX_QUEUE_SIZE=2), True),
    "fix_cp_none": ("db5", dict(FIX_CP=None), {}, True),
    "copy_all": ("db5", dict(COPY_ST_ONLY=False, SAMPLER_VAL=True), dict(MAX_QUEUE_SIZE=3), True),
    "no_gt_sampling": (None, {}, dict(TRANS_NOISE=2.0), True),
    "overlap": ("near", dict(DROPOUT=0.0), dict(TRANS_NOISE=2.0, ROT_NOISE=0.3), False),
}


def seed_of(case):
    return 5000 + list(CASES).index(case)


def augmentor_config(case, folder_frustum, folder_st):
    """the shipped DATA_AUGMENTOR (DISABLE_AUG_LIST ['placeholder']), varied by the case"""
    db, loader, queue, world = CASES[case]
    gt = GS.sampler_config("transfusion")
    if db is not None:
        gt['DB_INFO_PATH'] = [f"{db}_dbinfos.pkl"]
    frustum = EDict(NAME='load_frustum_pseudos', PSEUDO_PATH=folder_frustum, SELF_TRAIN_PATH=folder_st, KNOWN_CLASSES=list(KNOWN),
                    **{k: v for k, v in {**SHIPPED_LOADER, **loader}.items() if v is not None})
    cp = EDict(NAME='unknowns_copy_paste', **{**SHIPPED_QUEUE, **queue})
    ops = ([gt] if db is not None else []) + [frustum, EDict(NAME='load_selftrain_pseudos'), cp]
    ops += [EDict(o) for o in GS.WORLD_OPS] if world else []
    return EDict(DISABLE_AUG_LIST=['placeholder'], AUG_CONFIG_LIST=ops)


def trace(aug):
    """Wrap the augmentor's queue so that every frame leaves {'sampled': boxes gt_sampling added, 'copy': the loader's copy
    boxes, 'scene_rows': rows in front of the pasted ones, 'pasted': the pasted rows} in the returned list (one dict per forward)."""
    log = []

    def wrap(fn, name):
        def step(data_dict):
            if not log or log[-1].get('done'):
                log.append(dict(n_gt=data_dict['gt_boxes'].shape[0], sampled=np.zeros((0, 7), np.float32)))
            cur = log[-1]
            if name == 'unknowns_copy_paste':
                cur['scene_rows'] = data_dict['points'].shape[0]
                cur['copy'] = np.array(aug.pseudo_loader.copy_boxes, np.float32).reshape(-1, 8)
            out = fn(data_dict=data_dict)
            if name == 'gt_sampling':
                cur['sampled'] = np.array(out['gt_boxes'][cur['n_gt']:, :7], np.float32)
            if name == 'unknowns_copy_paste':
                cur['pasted'] = np.array(out['points'][cur['scene_rows']:], np.float32)
                cur['done'] = True
            return out
        return step

    names = [getattr(f, 'func', f).__name__ if hasattr(getattr(f, 'func', f), '__name__') else type(f).__name__ for f in
             aug.data_augmentor_queue]
    aug.data_augmentor_queue = [wrap(f, 'gt_sampling' if n in ('gt_sampling', 'DataBaseSampler') else n)
                                for f, n in zip(aug.data_augmentor_queue, names)]
    return log


def overlaps(entry):
    """(a copy box overlaps a sampled box in BEV, a pasted row lies inside a sampled box) of one traced frame"""
    from findnpropagate_amd.augmentor import database_sampler as DS
    from findnpropagate_amd.iou3d_nms import iou3d_nms_utils
    s, c = entry['sampled'], entry.get('copy', np.zeros((0, 8), np.float32))
    a = bool(s.shape[0] and c.shape[0] and (iou3d_nms_utils.boxes_bev_iou_cpu(c[:, :7].copy(), s.copy()) > 0).any())
    p = entry.get('pasted', np.zeros((0, 5), np.float32))
    b = bool(s.shape[0] and p.shape[0] and not DS.points_outside_boxes(p[:, :3], DS.cut_records(s)).all())
    return a, b
