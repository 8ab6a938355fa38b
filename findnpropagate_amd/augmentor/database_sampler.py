"""DataBaseSampler (pcdet/datasets/augmentor/database_sampler.py:15-150, :367-504): gt_sampling's lidar path.

Same constructor, data_dict keys, per-class pointer / indices state and np.random draws (np.random.permutation when a class's
pointer runs past its list): a seeded run draws the reference's samples.  The collision test is the rotated BEV IoU of the
library's host entry (iou3d_nms_utils.boxes_bev_iou_cpu -> fnp_host_boxes_iou_bev), quirks included: iou1 falls back to iou2
when the scene has no box, existed_boxes grows class by class, and gt_boxes_mask is applied only when something was sampled
(it is popped either way).  Runs in DataLoader workers: no device is used.

add_sampled_boxes_to_scene cuts the scene points that lie inside the sampled boxes enlarged by REMOVE_EXTRA_WIDTH
(box_utils.remove_points_in_boxes3d -> roiaware_pool3d points_in_boxes_cpu):
  host      (default) here, through fnp_host_points_outside_boxes: the reference's keep mask bit for bit, without its (M, N)
            matrix;
  deferred  (deferred=True) the object rows are put in front of the scene rows untested, and the cut is recorded for
            sparse.prepare_points: data_dict['prep_cut_boxes'] (M, 7) f32, the enlarged boxes as the host mode tests them, and
            data_dict['prep_cut_from'], the number of leading object rows (never cut).  The collate stacks them with
            data_augmentor.stack_cut_boxes.  A scene without data_dict['points'] and with data_dict['raw_sweeps'] (a
            datasets.nuscenes_sweeps.pack_sweeps scene that the device assembles) has no rows to put the object rows in front
            of: they are recorded in data_dict['prep_lead_rows'] ((n, 5) f32; (0, 5) when nothing is sampled) and travel as a
            finished-row sweep in front of the scene's sweeps (pack_sweeps(lead=)), whose window yields prep_cut_from on the card.
USE_ROAD_PLANE, IMG_AUG_TYPE, USE_SHARED_MEMORY, a true DATABASE_WITH_FAKELIDAR and the BACKUP_DB_INFO fallback (none of them in
the nuScenes configs) raise NotImplementedError naming the key.
"""
import pickle
from pathlib import Path

import numpy as np

from .. import lib as _l
from ..iou3d_nms import iou3d_nms_utils

CUT_BOXES_KEY = 'prep_cut_boxes'
CUT_FROM_KEY = 'prep_cut_from'
LEAD_ROWS_KEY = 'prep_lead_rows'
RAW_SWEEPS_KEY = 'raw_sweeps'
RAW_FEATURES = 5   # the columns of an assembled row: x, y, z, intensity, time lag


def _get(config, key, default=None):
    if isinstance(config, dict):
        return config.get(key, default)
    return getattr(config, key, default)


def cut_records(boxes):
    """(M, 7) boxes -> (M, 8) f32 records {cx, cy, cz, dx, dy, dz, cos(-h), sin(-h)} (fnp_host_cut_records: the C library's
    cosf / sinf, as points_in_boxes_cpu evaluates them)"""
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 7)
    out = np.empty((boxes.shape[0], 8), np.float32)
    if boxes.shape[0]:
        _l.check(_l.load().fnp_host_cut_records(boxes.ctypes.data, boxes.shape[0], out.ctypes.data), "fnp_host_cut_records")
    return out


def points_outside_boxes(points, records):
    """keep mask (N,) bool of the points (N, C) f32 that lie in none of the records (M, 8): remove_points_in_boxes3d's
    points_in_boxes_cpu(points[:, :3], boxes).sum(0) == 0 (fnp_host_points_outside_boxes)"""
    points = np.ascontiguousarray(points, np.float32)
    records = np.ascontiguousarray(records, np.float32).reshape(-1, 8)
    n, C = points.shape
    keep = np.empty((n,), np.uint8)
    rc = _l.load().fnp_host_points_outside_boxes(points.ctypes.data if n else None, n, C,
                                                 records.ctypes.data if records.shape[0] else None, records.shape[0],
                                                 keep.ctypes.data if n else None)
    _l.check(rc, "fnp_host_points_outside_boxes")
    return keep.view(np.bool_)


def enlarge_cut_boxes(boxes, extra_width):
    """box_utils.enlarge_box3d as remove_points_in_boxes3d receives it: check_numpy_to_torch casts the (M, 7) boxes to f32, the
    extents grow by the f32 extra width in f32"""
    large = np.array(boxes[:, 0:7], np.float32)
    large[:, 3:6] += np.asarray(extra_width, np.float32)[None, :]
    return large


class DataBaseSampler(object):
    def __init__(self, root_path, sampler_cfg, class_names, logger=None, deferred=False):
        self.root_path = root_path
        self.class_names = class_names
        self.sampler_cfg = sampler_cfg
        self.deferred = bool(deferred)
        for key, off in (('USE_ROAD_PLANE', False), ('IMG_AUG_TYPE', None), ('USE_SHARED_MEMORY', False),
                         ('DATABASE_WITH_FAKELIDAR', False)):
            if _get(sampler_cfg, key, off) not in (off, None, False):
                raise NotImplementedError(f"DataBaseSampler: {key} is not supported by this build")
        self.img_aug_type = None
        self.logger = logger
        self.db_infos = {}
        for class_name in class_names:
            self.db_infos[class_name] = []

        self.use_shared_memory = False

        for db_info_path in _get(sampler_cfg, 'DB_INFO_PATH'):
            db_info_path = Path(self.root_path).resolve() / db_info_path
            if not db_info_path.exists():
                if _get(sampler_cfg, 'BACKUP_DB_INFO') is not None:
                    raise NotImplementedError(f"DataBaseSampler: {db_info_path} is missing and the BACKUP_DB_INFO fallback "
                                              "is not supported by this build")
                raise FileNotFoundError(str(db_info_path))
            with open(str(db_info_path), 'rb') as f:
                infos = pickle.load(f)
                [self.db_infos[cur_class].extend(infos[cur_class]) for cur_class in class_names]

        for func_name, val in _get(sampler_cfg, 'PREPARE').items():
            self.db_infos = getattr(self, func_name)(self.db_infos, val)

        self.gt_database_data_key = None

        self.sample_groups = {}
        self.sample_class_num = {}
        self.limit_whole_scene = _get(sampler_cfg, 'LIMIT_WHOLE_SCENE', False)

        for x in _get(sampler_cfg, 'SAMPLE_GROUPS'):
            class_name, sample_num = x.split(':')
            if class_name not in class_names:
                continue
            self.sample_class_num[class_name] = sample_num
            self.sample_groups[class_name] = {
                'sample_num': sample_num,
                'pointer': len(self.db_infos[class_name]),
                'indices': np.arange(len(self.db_infos[class_name]))
            }

    def __getstate__(self):
        d = dict(self.__dict__)
        del d['logger']
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)

    def filter_by_difficulty(self, db_infos, removed_difficulty):
        new_db_infos = {}
        for key, dinfos in db_infos.items():
            pre_len = len(dinfos)
            new_db_infos[key] = [info for info in dinfos if info['difficulty'] not in removed_difficulty]
            if self.logger is not None:
                self.logger.info('Database filter by difficulty %s: %d => %d' % (key, pre_len, len(new_db_infos[key])))
        return new_db_infos

    def filter_by_min_points(self, db_infos, min_gt_points_list):
        for name_num in min_gt_points_list:
            name, min_num = name_num.split(':')
            min_num = int(min_num)
            if min_num > 0 and name in db_infos.keys():
                filtered_infos = []
                for info in db_infos[name]:
                    if info['num_points_in_gt'] >= min_num:
                        filtered_infos.append(info)
                if self.logger is not None:
                    self.logger.info('Database filter by min points %s: %d => %d' %
                                     (name, len(db_infos[name]), len(filtered_infos)))
                db_infos[name] = filtered_infos
        return db_infos

    def sample_with_fixed_number(self, class_name, sample_group):
        sample_num, pointer, indices = int(sample_group['sample_num']), sample_group['pointer'], sample_group['indices']
        if pointer >= len(self.db_infos[class_name]):
            indices = np.random.permutation(len(self.db_infos[class_name]))
            pointer = 0
        sampled_dict = [self.db_infos[class_name][idx] for idx in indices[pointer: pointer + sample_num]]
        pointer += sample_num
        sample_group['pointer'] = pointer
        sample_group['indices'] = indices
        return sampled_dict

    def _object_points(self, info):
        """the object's .bin file as f32 rows, as f64 when the f32 row count is not num_points_in_gt; moved to the box centre"""
        nf = _get(self.sampler_cfg, 'NUM_POINT_FEATURES')
        file_path = Path(self.root_path) / info['path']
        obj_points = np.fromfile(str(file_path), dtype=np.float32).reshape([-1, nf])
        if obj_points.shape[0] != info['num_points_in_gt']:
            obj_points = np.fromfile(str(file_path), dtype=np.float64).reshape(-1, nf)
        assert obj_points.shape[0] == info['num_points_in_gt']
        obj_points[:, :3] += info['box3d_lidar'][:3].astype(np.float32)
        return obj_points

    def add_sampled_boxes_to_scene(self, data_dict, sampled_gt_boxes, total_valid_sampled_dict):
        gt_boxes_mask = data_dict['gt_boxes_mask']
        gt_boxes = data_dict['gt_boxes'][gt_boxes_mask]
        gt_names = data_dict['gt_names'][gt_boxes_mask]
        raw = self.deferred and 'points' not in data_dict and RAW_SWEEPS_KEY in data_dict
        points = np.zeros((0, RAW_FEATURES), np.float32) if raw else data_dict['points']

        obj_points = np.concatenate([self._object_points(info) for info in total_valid_sampled_dict], axis=0)
        sampled_gt_names = np.array([x['name'] for x in total_valid_sampled_dict])

        by_time = _get(self.sampler_cfg, 'FILTER_OBJ_POINTS_BY_TIMESTAMP', False)
        if by_time or obj_points.shape[-1] != points.shape[-1]:
            if by_time:
                time_range = _get(self.sampler_cfg, 'TIME_RANGE')
                min_time = min(time_range[0], time_range[1])
                max_time = max(time_range[0], time_range[1])
            else:
                assert obj_points.shape[-1] == points.shape[-1] + 1
                min_time = max_time = 0.0   # multi-frame object points -> single-frame ones
            time_mask = np.logical_and(obj_points[:, -1] < max_time + 1e-6, obj_points[:, -1] > min_time - 1e-6)
            obj_points = obj_points[time_mask]

        large_sampled_gt_boxes = enlarge_cut_boxes(sampled_gt_boxes, _get(self.sampler_cfg, 'REMOVE_EXTRA_WIDTH'))
        obj_rows = obj_points[:, :points.shape[-1]]
        if self.deferred:
            data_dict[CUT_BOXES_KEY] = large_sampled_gt_boxes
            data_dict[CUT_FROM_KEY] = int(obj_rows.shape[0])
        else:   # (remove_points_in_boxes3d hands back its f32 copy of the points)
            points = np.asarray(points, np.float32)
            points = points[points_outside_boxes(points[:, 0:3], cut_records(large_sampled_gt_boxes))]
        gt_names = np.concatenate([gt_names, sampled_gt_names], axis=0)
        gt_boxes = np.concatenate([gt_boxes, sampled_gt_boxes], axis=0)
        data_dict['gt_boxes'] = gt_boxes
        data_dict['gt_names'] = gt_names
        if raw:
            data_dict[LEAD_ROWS_KEY] = np.ascontiguousarray(obj_rows, np.float32)
        else:
            data_dict['points'] = np.concatenate([obj_rows, points], axis=0)
        return data_dict

    def __call__(self, data_dict):
        gt_boxes = data_dict['gt_boxes']
        gt_names = data_dict['gt_names'].astype(str)
        existed_boxes = gt_boxes
        total_valid_sampled_dict = []
        if self.deferred:   # nothing to cut unless something is sampled
            data_dict[CUT_BOXES_KEY] = np.zeros((0, 7), np.float32)
            data_dict[CUT_FROM_KEY] = 0
            if 'points' not in data_dict and RAW_SWEEPS_KEY in data_dict:
                data_dict[LEAD_ROWS_KEY] = np.zeros((0, RAW_FEATURES), np.float32)

        for class_name, sample_group in self.sample_groups.items():
            if self.limit_whole_scene:
                num_gt = np.sum(class_name == gt_names)
                sample_group['sample_num'] = str(int(self.sample_class_num[class_name]) - num_gt)
            if int(sample_group['sample_num']) > 0:
                sampled_dict = self.sample_with_fixed_number(class_name, sample_group)
                sampled_boxes = np.stack([x['box3d_lidar'] for x in sampled_dict], axis=0).astype(np.float32)

                iou1 = iou3d_nms_utils.boxes_bev_iou_cpu(sampled_boxes[:, 0:7], existed_boxes[:, 0:7])
                iou2 = iou3d_nms_utils.boxes_bev_iou_cpu(sampled_boxes[:, 0:7], sampled_boxes[:, 0:7])
                iou2[range(sampled_boxes.shape[0]), range(sampled_boxes.shape[0])] = 0
                iou1 = iou1 if iou1.shape[1] > 0 else iou2
                valid_mask = ((iou1.max(axis=1) + iou2.max(axis=1)) == 0)

                valid_mask = valid_mask.nonzero()[0]
                valid_sampled_dict = [sampled_dict[x] for x in valid_mask]
                valid_sampled_boxes = sampled_boxes[valid_mask]

                existed_boxes = np.concatenate((existed_boxes, valid_sampled_boxes[:, :existed_boxes.shape[-1]]), axis=0)
                total_valid_sampled_dict.extend(valid_sampled_dict)

        sampled_gt_boxes = existed_boxes[gt_boxes.shape[0]:, :]

        if total_valid_sampled_dict.__len__() > 0:
            data_dict = self.add_sampled_boxes_to_scene(data_dict, sampled_gt_boxes, total_valid_sampled_dict)

        data_dict.pop('gt_boxes_mask')
        return data_dict
