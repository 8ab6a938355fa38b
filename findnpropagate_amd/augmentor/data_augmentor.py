"""DataAugmentor (pcdet/datasets/augmentor/data_augmentor.py:10-56,345-382) with the four world augmentations of the hot path's
config (transfusion_lidar.yaml:31-42): random_world_flip (:59-85), random_world_rotation (:87-108), random_world_scaling (:110-134)
and random_world_translation (:157-181), on top of the numbers of augmentor_utils.py:8-156.

Same constructor, DISABLE_AUG_LIST handling, np.random draws in the same order (flip x, flip y, uniform rotation, uniform scale,
three normals: a seeded run draws the reference's parameters), the same data_dict keys (flip_x, flip_y, noise_rot, noise_scale,
noise_translate) and the same box arithmetic, quirks included: pseudo_global_scaling scales x, y, z twice
(augmentor_utils.py:155-156), roi-box scaling leaves the gt velocities alone (:130-146), and forward() wraps the heading with
limit_period(offset=0.5, period=2 pi) at the end (:380-382).

Two modes:
  host      (default) the points are transformed here, in the reference's arithmetic — for DataLoader worker processes with
            no GPU.  The points' rotation is written out in the fused form of rotate_points_fused: what torch's CPU matmul
            computes on the reference's machine, what the device computes, and the same bits on any CPU;
  deferred  (deferred=True) only the boxes (tens of rows) are transformed here; the points are left as they are and the scene's
            op program is recorded in data_dict['prep_program'] ((K, 4) f32 rows {op, a, b, c}, one per drawn op in config
            order), for sparse.prepare_points to apply on the device in front of the voxeliser.  The collate stacks the
            programs with stack_programs() to (B, K, 4).
gt_sampling builds database_sampler.DataBaseSampler as the reference does (data_augmentor.py:42-49) and runs at its place in the
queue.  Host mode cuts the scene points inside the sampled boxes here; deferred mode puts the object rows in front of the scene
rows and records the cut (data_dict['prep_cut_boxes'], data_dict['prep_cut_from']) for sparse.prepare_points, which cuts before
it applies the program: a deferred gt_sampling after a recorded world op raises ValueError.  The collate stacks the cuts with
stack_cut_boxes().
load_frustum_pseudos, load_selftrain_pseudos and unknowns_copy_paste build and share one pseudo_loader.PseudoLoader with the
reference's constructor semantics (data_augmentor.py:327-360) and delegate to it.  The two load_* entries touch boxes only and
run the same in both modes.  unknowns_copy_paste feeds the sampler's queue from the scene and appends the pasted object rows
behind every scene row.  In deferred mode, after a deferred gt_sampling, the queue is fed only from the rows that survive the
pending cut (the rows below prep_cut_from, and the rows inside no cut box): host mode's cut scene, row for row, so the queue,
the np.random draws and the pasted rows are the host mode's.  It then records data_dict['prep_cut_to'], the rows in front of
the first pasted row, so that the device cut spares the pasted rows; stack_cut_boxes(..., cut_to_list) makes the 4-tuple cut
of sparse.prepare_points.  A deferred unknowns_copy_paste after a recorded world op raises ValueError.
RAW SCENES.  A deferred DataAugmentor also takes a scene that has no 'points' but data_dict['raw_sweeps'], a scene of
datasets.nuscenes_sweeps.pack_sweeps whose rows the device will assemble (sparse.assemble_sweeps): gt_sampling records its object
rows in data_dict['prep_lead_rows'] instead of putting them in front of rows that do not exist yet, unknowns_copy_paste obtains the
rows inside its copy boxes from the provider data_dict['scene_rows'] (nuscenes_sweeps.HostSceneRows, the default, or
DeviceSceneRows) and records the pasted rows in data_dict['prep_tail_rows']; the queue logic, the np.random draws, the boxes and
the programme are those of the host mode on the assembled scene.  forward is forward_head then forward_tail: forward_head runs the
entries in front of the first one that needs scene rows (file reads, gt_sampling, the two load_*: a DataLoader worker can run it),
forward_tail the rest and the epilogue, in the process that owns the device — and with it the copy-paste queue, which then lives
in that one process.  The order of work for a batch is in INTEGRATION.md.
Any other augmentor (random_local_*, frustum dropout, image ops) raises NotImplementedError naming itself, unless
DISABLE_AUG_LIST lists it.
"""
from functools import partial

import numpy as np
import torch

from . import database_sampler
from .pseudo_loader import TAIL_ROWS_KEY, PseudoLoader, rotate_points_along_z

OP_NONE, OP_FLIP_X, OP_FLIP_Y, OP_ROTATE, OP_SCALE, OP_TRANSLATE = range(6)
MAX_STEPS = 6   # FNP_PREP_MAX_STEPS (include/fnp.h)
PROGRAM_KEY = 'prep_program'
CUT_TO_KEY = 'prep_cut_to'
CUT_TO_END = 0x7fffffff   # a cut_to that reaches the end of the scene
RAW_SWEEPS_KEY = database_sampler.RAW_SWEEPS_KEY
LEAD_ROWS_KEY = database_sampler.LEAD_ROWS_KEY
SCENE_ROWS_KEY = 'scene_rows'
COPY_STATE_KEY = 'prep_copy_state'   # forward_head -> forward_tail: the loader's copy boxes of this frame
NEEDS_SCENE_ROWS = ('unknowns_copy_paste',)
SUPPORTED = ('gt_sampling', 'load_frustum_pseudos', 'load_selftrain_pseudos', 'unknowns_copy_paste', 'random_world_flip',
             'random_world_rotation', 'random_world_scaling', 'random_world_translation')


def limit_period(val, offset=0.5, period=np.pi):
    """common_utils.py:21-24 (f32 torch arithmetic; numpy in -> numpy out)."""
    is_numpy = isinstance(val, np.ndarray)
    v = torch.from_numpy(val).float() if is_numpy else val
    ans = v - torch.floor(v / period + offset) * period
    return ans.numpy() if is_numpy else ans


def rotation_cos_sin(angle):
    """cos, sin of the f32 angle as rotate_points_along_z computes them (torch, f32): the rotation row of a program."""
    a = torch.from_numpy(np.array([angle])).float()
    return np.float32(torch.cos(a)[0].item()), np.float32(torch.sin(a)[0].item())


def _fma32(a, b, c):
    """f32 a*b + c with ONE rounding (numpy has no fused multiply-add): the product is exact in f64 (24 + 24 bits), TwoSum gives
    the f64 sum and its error, and the error decides the one case where rounding the f64 sum to f32 goes wrong — a sum exactly
    halfway between two f32 values."""
    p = a.astype(np.float64) * np.float64(b)
    q = np.asarray(c, np.float64)
    s = p + q
    bb = s - p
    e = (p - (s - bb)) + (q - bb)
    r = s.astype(np.float32)
    rd = r.astype(np.float64)
    other = np.nextafter(r, np.where(s > rd, np.float32(np.inf), np.float32(-np.inf)))   # the f32 on the other side of s
    tie = (e != 0) & (s != rd) & (s == (rd + other.astype(np.float64)) * 0.5)
    return np.where(tie & ((r < s) == (e > 0)), other, r)


def rotate_points_fused(points, angle):
    """random_world_rotation of the points: rotate_points_along_z's f32 [x y z] @ [[c s 0] [-s c 0] [0 0 1]] in the rounding
    torch's CPU matmul gives it for point clouds on the reference's machine — x' = fma(y, -s, x*c), y' = fma(y, c, x*s), z and
    the other columns as they are (tests/golden/augment_golden.npz).  Written out because a CPU matmul's rounding is the BLAS
    kernel's choice (another CPU model was seen to round some points differently in the last place); this form is what the
    device computes.  The boxes (tens of rows, another matmul path) keep rotate_points_along_z itself."""
    c, s = rotation_cos_sin(angle)
    out = points.astype(np.float32, copy=True)
    x, y = out[:, 0].copy(), out[:, 1].copy()
    out[:, 0] = _fma32(y, -s, x * c)
    out[:, 1] = _fma32(y, c, x * s)
    return out


def stack_programs(programs, steps=None):
    """Collate: per-scene (K_b, 4) programs -> (B, K, 4) f32, shorter ones padded with no-op rows (K = max K_b or `steps`)."""
    K = max([p.shape[0] for p in programs] + [0]) if steps is None else int(steps)
    if K > MAX_STEPS:
        raise ValueError(f"a point program holds at most {MAX_STEPS} steps, got {K}")
    out = np.zeros((len(programs), K, 4), np.float32)
    for b, p in enumerate(programs):
        out[b, :p.shape[0]] = p
    return out


def stack_cut_boxes(boxes_list, cut_from_list, cut_to_list=None):
    """Collate: per-scene enlarged cut boxes (M_b, 7) and leading object row counts -> records (sum M_b, 8) f32
    (fnp_host_cut_records), box offsets (B+1,) int32 and cut_from (B,) int32: the `cut` of sparse.prepare_points.
    With cut_to_list (per scene data_dict['prep_cut_to'], or None where the scene recorded none), also cut_to (B,) int32, None
    -> CUT_TO_END: the 4-tuple cut."""
    boxes = [np.asarray(b, np.float32).reshape(-1, 7) for b in boxes_list]
    off = np.zeros(len(boxes) + 1, np.int32)
    off[1:] = np.cumsum([b.shape[0] for b in boxes])
    records = database_sampler.cut_records(np.concatenate(boxes, 0) if boxes else np.zeros((0, 7), np.float32))
    cut_from = np.asarray(cut_from_list, np.int32).reshape(len(boxes))
    if cut_to_list is None:
        return records, off, cut_from
    cut_to = np.array([CUT_TO_END if t is None else int(t) for t in cut_to_list], np.int32).reshape(len(boxes))
    return records, off, cut_from, cut_to


def _get(config, key, default=None):
    if isinstance(config, dict):
        return config.get(key, default)
    return getattr(config, key, default)


def _flip_x(boxes, enable):
    """random_flip_along_x on boxes: y, heading and (with velocities) vy change sign."""
    if enable:
        boxes[:, 1] = -boxes[:, 1]
        boxes[:, 6] = -boxes[:, 6]
        if boxes.shape[1] > 7:
            boxes[:, 8] = -boxes[:, 8]
    return boxes


def _flip_y(boxes, enable):
    """random_flip_along_y on boxes: x and (with velocities) vx change sign, heading -> -(heading + pi)."""
    if enable:
        boxes[:, 0] = -boxes[:, 0]
        boxes[:, 6] = -(boxes[:, 6] + np.pi)
        if boxes.shape[1] > 7:
            boxes[:, 7] = -boxes[:, 7]
    return boxes


def _rotate_boxes(boxes, rot):
    """global_rotation on boxes: centres about z, heading + rot, velocities (as xy0 rows)."""
    angle = np.array([rot])
    boxes[:, 0:3] = rotate_points_along_z(boxes[np.newaxis, :, 0:3], angle)[0]
    boxes[:, 6] += rot
    if boxes.shape[1] > 7:
        vel = np.hstack((boxes[:, 7:9], np.zeros((boxes.shape[0], 1))))
        boxes[:, 7:9] = rotate_points_along_z(vel[np.newaxis, :, :], angle)[0][:, 0:2]
    return boxes


class DataAugmentor(object):
    def __init__(self, root_path, augmentor_configs, class_names, logger=None, deferred=False):
        self.root_path = root_path
        self.class_names = class_names
        self.logger = logger
        self.deferred = bool(deferred)
        self.data_augmentor_queue = []
        self._build_queue(augmentor_configs)

    def _build_queue(self, augmentor_configs):
        self.data_augmentor_queue = []
        self.queue_names = []
        is_list = isinstance(augmentor_configs, list)
        cfg_list = augmentor_configs if is_list else _get(augmentor_configs, 'AUG_CONFIG_LIST')
        disabled = [] if is_list else (_get(augmentor_configs, 'DISABLE_AUG_LIST', None) or [])
        for cur_cfg in cfg_list:
            name = _get(cur_cfg, 'NAME')
            if name in disabled:
                continue
            if name not in SUPPORTED:
                raise NotImplementedError(f"DataAugmentor.{name} is not implemented in this build (list it in DISABLE_AUG_LIST)")
            self.data_augmentor_queue.append(getattr(self, name)(config=cur_cfg))
            self.queue_names.append(name)

    def disable_augmentation(self, augmentor_configs):
        self._build_queue(augmentor_configs)

    def __getstate__(self):
        d = dict(self.__dict__)
        del d['logger']
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)

    def gt_sampling(self, data_dict=None, config=None):
        if data_dict is None:
            if self.root_path is None or _get(config, 'DB_INFO_PATH') is None:
                raise NotImplementedError("DataAugmentor.gt_sampling needs a database: root_path and DB_INFO_PATH")
            db_sampler = database_sampler.DataBaseSampler(root_path=self.root_path, sampler_cfg=config,
                                                          class_names=self.class_names, logger=self.logger,
                                                          deferred=self.deferred)
            return partial(self.gt_sampling, config=db_sampler)
        if self.deferred and PROGRAM_KEY in data_dict:
            raise ValueError("a deferred gt_sampling must come before the world ops: the device cuts the scene points "
                             "before it applies their program")
        return config(data_dict)

    def _pseudo_loader(self, config):
        """PseudoLoader(...) of a load_* entry: the reference's keyword mapping and defaults (data_augmentor.py:329-334)"""
        return PseudoLoader(known_class_names=_get(config, 'KNOWN_CLASSES'), pseudo_path=_get(config, 'PSEUDO_PATH'),
                            self_train_path=_get(config, 'SELF_TRAIN_PATH', None), dropout=_get(config, 'DROPOUT', 0.5),
                            min_score=_get(config, 'MIN_SCORE', None), pseudo_nms_thresh=_get(config, 'PSEUDO_NMS_THRESH', 0.1),
                            max_selftrain_per_class=_get(config, 'MAX_SELFTRAIN_PER_CLASS', None),
                            fix_cp=_get(config, 'FIX_CP', None), mom=_get(config, 'MOMENTUM', 0.9),
                            copy_st_only=_get(config, 'COPY_ST_ONLY', False), sampler_val=_get(config, 'SAMPLER_VAL', True))

    def load_frustum_pseudos(self, data_dict=None, config=None):
        if data_dict is None:
            self.pseudo_loader = self._pseudo_loader(config)
            return partial(self.load_frustum_pseudos, config=config)
        return self.pseudo_loader.load_frustum_pseudos(data_dict)

    def load_selftrain_pseudos(self, data_dict=None, config=None):
        if data_dict is None:
            if getattr(self, 'pseudo_loader', None) is None:   # no frustum pseudos: this entry builds the loader
                self.pseudo_loader = self._pseudo_loader(config)
            return partial(self.load_selftrain_pseudos, config=config)
        return self.pseudo_loader.load_selftrain_pseudos(data_dict)

    def unknowns_copy_paste(self, data_dict=None, config=None):
        if data_dict is None:
            loader = getattr(self, 'pseudo_loader', None)
            if loader is None:   # (the reference fails here with an AttributeError)
                raise AttributeError("DataAugmentor.unknowns_copy_paste needs a pseudo loader: list load_frustum_pseudos or "
                                     "load_selftrain_pseudos before it")
            sampler = loader.sampler
            sampler.max_queue_size_per_class = _get(config, 'MAX_QUEUE_SIZE', sampler.max_queue_size_per_class)
            sampler.queue_metric = _get(config, 'QUEUE_METRIC', sampler.queue_metric)
            sampler.trans_noise = _get(config, 'TRANS_NOISE', sampler.trans_noise)
            sampler.rot_noise = _get(config, 'ROT_NOISE', sampler.rot_noise)
            sampler.timestamp = _get(config, 'TIMESTAMP', sampler.timestamp)
            return partial(self.unknowns_copy_paste, config=config)
        if self.deferred and PROGRAM_KEY in data_dict:
            raise ValueError("a deferred unknowns_copy_paste must come before the world ops: the rows it appends are not "
                             "transformed, and the program applies to every row")
        if self.deferred and 'points' not in data_dict and RAW_SWEEPS_KEY in data_dict:
            provider = data_dict.get(SCENE_ROWS_KEY)
            if provider is None:   # no device in this process: the host assembly answers
                from ..datasets.nuscenes_sweeps import HostSceneRows
                provider = HostSceneRows(data_dict[RAW_SWEEPS_KEY], lead=data_dict.get(LEAD_ROWS_KEY))
            cut_boxes = data_dict.get(database_sampler.CUT_BOXES_KEY)
            return self.pseudo_loader.copy_and_paste(data_dict, rows=lambda boxes7: provider(boxes7, cut_boxes))
        if not (self.deferred and database_sampler.CUT_BOXES_KEY in data_dict):
            return self.pseudo_loader.copy_and_paste(data_dict)
        n_scene = int(data_dict['points'].shape[0])
        cut = (database_sampler.cut_records(data_dict[database_sampler.CUT_BOXES_KEY]),
               int(data_dict[database_sampler.CUT_FROM_KEY]), n_scene)
        data_dict = self.pseudo_loader.copy_and_paste(data_dict, cut=cut)
        data_dict[CUT_TO_KEY] = n_scene
        return data_dict

    def _points(self, data_dict):
        """the scene's points; None for a raw scene of the deferred mode, whose rows are not assembled yet"""
        if self.deferred and 'points' not in data_dict and RAW_SWEEPS_KEY in data_dict:
            return None
        return data_dict['points']

    def _record(self, data_dict, op, a=0.0, b=0.0, c=0.0):
        """deferred mode: append one step to the scene's program"""
        row = np.array([[op, a, b, c]], np.float32)
        prog = data_dict.get(PROGRAM_KEY)
        prog = row if prog is None else np.concatenate([prog, row])
        if prog.shape[0] > MAX_STEPS:
            raise ValueError(f"a point program holds at most {MAX_STEPS} steps")
        data_dict[PROGRAM_KEY] = prog

    def random_world_flip(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.random_world_flip, config=config)
        gt_boxes, points = data_dict['gt_boxes'], self._points(data_dict)
        for cur_axis in config['ALONG_AXIS_LIST']:
            assert cur_axis in ['x', 'y']
            enable = np.random.choice([False, True], replace=False, p=[0.5, 0.5])
            flip = _flip_x if cur_axis == 'x' else _flip_y
            gt_boxes = flip(gt_boxes, enable)
            if self.deferred:
                self._record(data_dict, (OP_FLIP_X if cur_axis == 'x' else OP_FLIP_Y) if enable else OP_NONE)
            elif enable:
                col = 1 if cur_axis == 'x' else 0
                points[:, col] = -points[:, col]
            data_dict['flip_%s' % cur_axis] = enable
            if 'roi_boxes' in data_dict.keys():
                num_frame, num_rois, dim = data_dict['roi_boxes'].shape
                data_dict['roi_boxes'] = flip(data_dict['roi_boxes'].reshape(-1, dim), enable).reshape(num_frame, num_rois, dim)
            if 'pseudo_boxes' in data_dict.keys():
                pb = data_dict['pseudo_boxes']
                if enable:   # pseudo_random_flip_along_*: no velocity columns
                    if cur_axis == 'x':
                        pb[:, 1] = -pb[:, 1]
                        pb[:, 6] = -pb[:, 6]
                    else:
                        pb[:, 0] = -pb[:, 0]
                        pb[:, 6] = -(pb[:, 6] + np.pi)
                data_dict['pseudo_boxes'] = pb
        data_dict['gt_boxes'] = gt_boxes
        if points is not None:
            data_dict['points'] = points
        return data_dict

    def random_world_rotation(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.random_world_rotation, config=config)
        rot_range = config['WORLD_ROT_ANGLE']
        if not isinstance(rot_range, list):
            rot_range = [-rot_range, rot_range]
        noise_rot = np.random.uniform(rot_range[0], rot_range[1])
        points = self._points(data_dict)
        if self.deferred:
            self._record(data_dict, OP_ROTATE, *rotation_cos_sin(noise_rot))
        else:
            points = rotate_points_fused(points, noise_rot)
        gt_boxes = _rotate_boxes(data_dict['gt_boxes'], noise_rot)
        if 'roi_boxes' in data_dict.keys():
            num_frame, num_rois, dim = data_dict['roi_boxes'].shape
            data_dict['roi_boxes'] = _rotate_boxes(data_dict['roi_boxes'].reshape(-1, dim), noise_rot).reshape(num_frame, num_rois, dim)
        if 'pseudo_boxes' in data_dict.keys():   # pseudo_global_rotation: centres and heading only
            pb = data_dict['pseudo_boxes']
            pb[:, 0:3] = rotate_points_along_z(pb[np.newaxis, :, 0:3], np.array([noise_rot]))[0]
            pb[:, 6] += noise_rot
            data_dict['pseudo_boxes'] = pb
        data_dict['gt_boxes'] = gt_boxes
        if points is not None:
            data_dict['points'] = points
        data_dict['noise_rot'] = noise_rot
        return data_dict

    def random_world_scaling(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.random_world_scaling, config=config)
        scale_range = config['WORLD_SCALE_RANGE']
        if scale_range[1] - scale_range[0] < 1e-3:
            # the reference returns two values here where its caller unpacks three (augmentor_utils.py:119-120)
            raise ValueError("random_world_scaling: WORLD_SCALE_RANGE narrower than 1e-3")
        noise_scale = np.random.uniform(scale_range[0], scale_range[1])
        gt_boxes, points = data_dict['gt_boxes'], self._points(data_dict)
        if self.deferred:
            self._record(data_dict, OP_SCALE, np.float32(noise_scale))
        else:
            points[:, :3] *= noise_scale
        gt_boxes[:, :6] *= noise_scale
        if 'roi_boxes' in data_dict.keys():   # global_scaling_with_roi_boxes: the gt velocities stay as they are
            data_dict['roi_boxes'][:, :, [0, 1, 2, 3, 4, 5, 7, 8]] *= noise_scale
        elif gt_boxes.shape[1] > 7:
            gt_boxes[:, 7:] *= noise_scale
        if 'pseudo_boxes' in data_dict.keys():   # pseudo_global_scaling: x, y, z twice (sic)
            pb = data_dict['pseudo_boxes']
            pb[:, :3] *= noise_scale
            pb[:, :6] *= noise_scale
            data_dict['pseudo_boxes'] = pb
        data_dict['gt_boxes'] = gt_boxes
        if points is not None:
            data_dict['points'] = points
        data_dict['noise_scale'] = noise_scale
        return data_dict

    def random_world_translation(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.random_world_translation, config=config)
        std = config['NOISE_TRANSLATE_STD']
        assert len(std) == 3
        draws = [np.random.normal(0, std[0], 1), np.random.normal(0, std[1], 1), np.random.normal(0, std[2], 1)]
        noise_translate = np.array(draws, dtype=np.float32).T   # (1, 3) f32
        gt_boxes, points = data_dict['gt_boxes'], self._points(data_dict)
        if self.deferred:
            self._record(data_dict, OP_TRANSLATE, *noise_translate[0])
        else:
            points[:, :3] += noise_translate
        gt_boxes[:, :3] += noise_translate
        if 'pseudo_boxes' in data_dict.keys():
            data_dict['pseudo_boxes'][:, :3] += noise_translate
        if 'roi_boxes' in data_dict.keys():
            data_dict['roi_boxes'][:, :3] += noise_translate
        data_dict['gt_boxes'] = gt_boxes
        if points is not None:
            data_dict['points'] = points
        data_dict['noise_translate'] = noise_translate
        return data_dict

    def _split(self):
        """index of the first queue entry that needs the scene rows (the queue's length when none does)"""
        names = getattr(self, 'queue_names', None) or []
        return next((k for k, n in enumerate(names) if n in NEEDS_SCENE_ROWS), len(self.data_augmentor_queue))

    def forward_head(self, data_dict):
        """The entries in front of the first one that needs scene rows: file reads, gt_sampling, the two load_*.  Needs no
        device and no assembled rows; what the loader keeps of this frame for unknowns_copy_paste travels in the data_dict."""
        for cur_augmentor in self.data_augmentor_queue[:self._split()]:
            data_dict = cur_augmentor(data_dict=data_dict)
        loader = getattr(self, 'pseudo_loader', None)
        if loader is not None:
            data_dict[COPY_STATE_KEY] = (loader.copy_boxes, loader.copy_scores, loader.pseudo_types)
        return data_dict

    def forward_tail(self, data_dict):
        """The rest of the queue, then the reference's epilogue (data_augmentor.py:374-398): in the process that owns the
        copy-paste queue (and, for raw scenes answered by DeviceSceneRows, the device)."""
        state = data_dict.pop(COPY_STATE_KEY, None)
        if state is not None:
            self.pseudo_loader.copy_boxes, self.pseudo_loader.copy_scores, self.pseudo_loader.pseudo_types = state
        for cur_augmentor in self.data_augmentor_queue[self._split():]:
            data_dict = cur_augmentor(data_dict=data_dict)
        data_dict.pop('pseudo_scores', None)
        data_dict['gt_boxes'][:, 6] = limit_period(data_dict['gt_boxes'][:, 6], offset=0.5, period=2 * np.pi)
        data_dict.pop('road_plane', None)
        if 'gt_boxes_mask' in data_dict:
            gt_boxes_mask = data_dict.pop('gt_boxes_mask')
            data_dict['gt_boxes'] = data_dict['gt_boxes'][gt_boxes_mask]
            data_dict['gt_names'] = data_dict['gt_names'][gt_boxes_mask]
            if 'gt_boxes2d' in data_dict:
                data_dict['gt_boxes2d'] = data_dict['gt_boxes2d'][gt_boxes_mask]
        return data_dict

    def forward(self, data_dict):
        """Run the queue, then the reference's epilogue (data_augmentor.py:374-398): forward_head, then forward_tail."""
        return self.forward_tail(self.forward_head(data_dict))
