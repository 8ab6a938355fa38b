"""Multi-sweep point clouds of a nuScenes sample (NuScenesDataset.get_sweep / get_lidar_with_sweeps,
pcdet/datasets/nuscenes/nuscenes_dataset.py:88-121), for the device: the sweep files are read and PACKED on the host, and
sparse.assemble_sweeps drops the ego returns, moves every sweep into the key frame and appends the time lag on the card.

  get_sweep, get_lidar_with_sweeps   the reference's arithmetic on arrays that are already read (numpy, host): the yardstick of
                                     the device path, and the host path of a worker that has no device
  pack_sweeps                        a batch of scenes -> the six arrays of sparse.assemble_sweeps; with lead / tail rows
                                     (gt_sampling's object rows, unknowns_copy_paste's pasted rows) as finished-row sweeps around
                                     each scene, and then a seventh array, the cut window
  HostSceneRows, DeviceSceneRows     the scene-row providers of a deferred DataAugmentor on raw scenes (data_dict['scene_rows']):
                                     the rows inside unknowns_copy_paste's copy boxes, from the host assembly or from one scene
                                     of a batch assembled on the card
  NuScenesSweepLoader                the file side: the reference's two methods with their signatures and their draw from
                                     numpy's global stream, and load_raw, which consumes the same draw and returns the raw
                                     sweeps for pack_sweeps

A scene, for pack_sweeps, is a list of sweeps (raw (n, 5) f32 as read from disk, matrix (4, 4) f64 or None, time_lag, is_key) in
the order their rows are wanted: the key frame first, then the drawn sweeps.  A key frame is neither filtered nor moved and its
lag is 0, whatever its tuple carries.

THE ORDER OF WORK with gt_sampling and unknowns_copy_paste in the queue (augmentor.data_augmentor, deferred mode, raw scenes):
  1. workers: load_raw, DataAugmentor.forward_head (records data_dict['prep_lead_rows'], data_dict['prep_cut_boxes']);
  2. the device process: pack_sweeps(scenes, lead=lead rows) WITHOUT tails, sparse.assemble_sweeps(..., window=window): the
     batch on the card, with cut_from / cut_to per scene;
  3. per scene, in batch order: data_dict['scene_rows'] = DeviceSceneRows(assembled, b), DataAugmentor.forward_tail (the
     copy-paste queue lives in this one process; records data_dict['prep_tail_rows'] and the programme);
  4. the pasted rows (a few hundred per scene) are staged behind the scene rows by assembling a second time with
     pack_sweeps(scenes, lead=, tail=): the same launches over the same raw rows plus the tails, no extra kernel and no row
     shuffling on the host;
  5. sparse.prepare_points(cut=(records, box_offsets, cut_from, cut_to)) with the second assembly's cut_from / cut_to."""
import os

import numpy as np

DROP_EGO = 1      # FNP_SWEEP_DROP_EGO
TRANSFORM = 2     # FNP_SWEEP_TRANSFORM
FINISHED = 4      # FNP_SWEEP_FINISHED: finished (x, y, z, intensity, lag) rows, taken as they are (assemble_sweeps with a window)


def check_flags(flags):
    """a finished-row sweep is neither filtered nor moved: FINISHED excludes DROP_EGO and TRANSFORM"""
    flags = np.asarray(flags)
    bad = (flags & FINISHED != 0) & (flags & (DROP_EGO | TRANSFORM) != 0)
    assert not bad.any(), f"sweeps {np.nonzero(bad)[0].tolist()}: FINISHED together with DROP_EGO or TRANSFORM"
    return flags


def ego_returns(xyzi, center_radius=1.0):
    """True for the returns from the ego vehicle itself: inside the square |x| < r, |y| < r, both ends strict, on the f32 values
    (get_sweep's remove_ego_points, nuscenes_dataset.py:89-91, keeps the others)."""
    inside_x = np.abs(xyzi[:, 0]) < center_radius
    inside_y = np.abs(xyzi[:, 1]) < center_radius
    return inside_x & inside_y


def get_sweep(points_raw, transform_matrix, time_lag, center_radius=1.0):
    """One sweep behind its file read (NuScenesDataset.get_sweep, nuscenes_dataset.py:88-102): points_raw (n, 5) f32 -> (xyzi
    (m, 4) f32, lag (m, 1) f64) with the ego returns gone and x, y, z moved by transform_matrix unless it is None.
    What fixes the bits: the move is ONE numpy dot of the (4, 4) f64 matrix with the (4, m) f64 array [x; y; z; 1] — numpy hands
    it to its BLAS — and its first three rows are stored into the f32 rows (one rounding); the lag column is f64 here and is cast
    where the sweeps are joined."""
    xyzi = np.asarray(points_raw, dtype=np.float32).reshape(-1, 5)[:, :4]
    kept = xyzi[~ego_returns(xyzi, center_radius)]                 # (m, 4) f32, a copy
    m = kept.shape[0]
    if transform_matrix is not None:
        homogeneous = np.ones((4, m), np.float64)
        homogeneous[:3] = kept[:, :3].T
        kept[:, :3] = transform_matrix.dot(homogeneous)[:3].T
    return kept, np.full((m, 1), time_lag, np.float64)


def get_lidar_with_sweeps(key_raw, sweeps, center_radius=1.0):
    """A sample behind its file reads and its draw (NuScenesDataset.get_lidar_with_sweeps, nuscenes_dataset.py:104-121): key_raw
    (n, 5) f32 and the drawn sweeps, in order, as (raw (n, 5) f32, matrix or None, time_lag) -> (N, 5) f32 [x, y, z, intensity,
    time lag].  The key frame is taken as it is, with lag 0; every lag goes from f64 to f32 in the store."""
    key = np.asarray(key_raw, dtype=np.float32).reshape(-1, 5)[:, :4]
    blocks = [(key, np.zeros((key.shape[0], 1), np.float64))]
    blocks += [get_sweep(raw, matrix, time_lag, center_radius) for raw, matrix, time_lag in sweeps]
    out = np.empty((sum(b[0].shape[0] for b in blocks), 5), np.float32)
    row = 0
    for xyzi, lag in blocks:
        out[row:row + xyzi.shape[0], :4] = xyzi
        out[row:row + xyzi.shape[0], 4:] = lag
        row += xyzi.shape[0]
    return out


def assemble_host(scene, center_radius=1.0):
    """get_lidar_with_sweeps of one scene in pack_sweeps' form (the key frame first)."""
    assert scene and scene[0][3], "a scene starts with its key frame"
    assert not any(s[3] for s in scene[1:]), "one key frame per scene"
    return get_lidar_with_sweeps(scene[0][0], [(raw, m, lag) for raw, m, lag, _ in scene[1:]], center_radius)


def pack_sweeps(scenes, device=None, lead=None, tail=None):
    """scenes: a list of scenes, each a list of (raw (n, 5) f32, matrix (4, 4) f64 or None, time_lag, is_key).
    Returns (raw (R, 5) f32, sweep_offsets (T+1,) int32, scene_sweeps (B+1,) int32, xform (T, 12) f64, flags (T,) int32,
    time_lag (T,) f32): the arguments of sparse.assemble_sweeps in their order.  numpy arrays; with a device, host torch tensors,
    pinned when the device is a GPU, for `t.to(device, non_blocking=True)`.
    time_lag goes through np.float32, which is what the reference's .astype(points.dtype) makes of its f64 column.
    lead, tail: None, or per scene (n, 5) f32 finished rows (x, y, z, intensity, lag) or None: they become a FINISHED sweep in
    front of and behind the scene's own sweeps (gt_sampling's data_dict['prep_lead_rows'], unknowns_copy_paste's
    data_dict['prep_tail_rows']).  When either is given a seventh array follows: window (B, 2) int32, per scene the range
    [first, end) of its own sweeps among the T sweeps, the rows that gt_sampling's cut may drop (assemble_sweeps(window=))."""
    B = len(scenes)
    windowed = lead is not None or tail is not None
    lead = [None] * B if lead is None else list(lead)
    tail = [None] * B if tail is None else list(tail)
    assert len(lead) == B and len(tail) == B, "lead and tail: one entry per scene"
    rows = [0]
    scene_sweeps = np.zeros(B + 1, np.int32)
    window = np.zeros((B, 2), np.int32)
    xform, flags, lag, parts = [], [], [], []

    def add(raw, flag=0, matrix=None, time_lag=0.0):
        raw = np.asarray(raw)
        assert raw.dtype == np.float32 and raw.ndim == 2 and raw.shape[1] == 5, "a sweep is (n, 5) float32 as read from disk"
        parts.append(raw)
        rows.append(rows[-1] + raw.shape[0])
        flags.append(flag)
        lag.append(np.float32(time_lag))
        xform.append(np.zeros(12, np.float64) if matrix is None else matrix)

    for b, scene in enumerate(scenes):
        if lead[b] is not None:
            add(lead[b], FINISHED)
        window[b, 0] = len(flags)
        for raw, matrix, time_lag, is_key in scene:
            if is_key:
                add(raw)
            elif matrix is None:
                add(raw, DROP_EGO, None, time_lag)
            else:
                m = np.asarray(matrix, np.float64)
                assert m.shape == (4, 4)
                add(raw, DROP_EGO | TRANSFORM, m[:3].reshape(12), time_lag)
        window[b, 1] = len(flags)
        if tail[b] is not None:
            add(tail[b], FINISHED)
        scene_sweeps[b + 1] = len(flags)
    assert rows[-1] <= np.iinfo(np.int32).max
    T = len(flags)
    raw = np.ascontiguousarray(np.concatenate(parts, 0)) if parts else np.zeros((0, 5), np.float32)
    out = (raw, np.asarray(rows, np.int32), scene_sweeps, np.asarray(xform, np.float64).reshape(T, 12),
           check_flags(np.asarray(flags, np.int32).reshape(T)), np.asarray(lag, np.float32).reshape(T))
    if windowed:
        out += (window,)
    if device is None:
        return out
    import torch

    pin = torch.device(device).type == "cuda"
    return tuple(torch.from_numpy(a).pin_memory() if pin else torch.from_numpy(a) for a in out)


def _rows5(rows):
    return np.zeros((0, 5), np.float32) if rows is None else np.ascontiguousarray(rows, np.float32).reshape(-1, 5)


class HostSceneRows:
    """data_dict['scene_rows'] from the host assembly of one scene (assemble_host + fnp_host_points_in_boxes_compact): for a
    process without a device, and the yardstick of DeviceSceneRows.  lead: gt_sampling's data_dict['prep_lead_rows'], which lie
    in front of the scene rows and are never cut."""

    def __init__(self, scene, lead=None, center_radius=1.0):
        lead = _rows5(lead)
        rows = assemble_host(scene, center_radius)
        self.window = (lead.shape[0], lead.shape[0] + rows.shape[0])
        self.points = np.concatenate([lead, rows], 0)

    def __call__(self, boxes7, cut_boxes=None):
        """boxes7 (T, 7), cut_boxes (M, 7) or None: gt_sampling's pending cut boxes -> (counts (T,) int64, the raw rows inside,
        box after box in row order (K, 5) f32), without the scene rows that the cut will drop"""
        from ..augmentor import database_sampler as DS
        from ..augmentor.pseudo_loader import points_in_boxes_compact
        cut = None
        if cut_boxes is not None and len(cut_boxes):
            cut = (DS.cut_records(cut_boxes), self.window[0], self.window[1])
        counts, idx, _ = points_in_boxes_compact(self.points, boxes7, cut=cut)
        return counts, self.points[idx]


class DeviceSceneRows:
    """data_dict['scene_rows'] from scene b of a batch assembled on the card (sparse.assemble_sweeps with a window: `assembled`
    is its dict): one sparse.rows_in_boxes launch sequence and one small device-to-host copy per call.  The lead rows are part of
    the assembly and its cut_from / cut_to bound the pending cut."""

    def __init__(self, assembled, b, capacity=4096):
        self.assembled, self.b, self.capacity = assembled, int(b), int(capacity)

    def __call__(self, boxes7, cut_boxes=None):
        import torch

        from .. import sparse as S
        from ..augmentor import database_sampler as DS
        a, b = self.assembled, self.b
        B, dev = a["batch_size"], a["points"].device

        def scene_only(boxes):
            rec = DS.cut_records(np.zeros((0, 7), np.float32) if boxes is None else boxes)
            off = np.zeros(B + 1, np.int32)
            off[b + 1:] = rec.shape[0]
            return torch.from_numpy(rec).to(dev), torch.from_numpy(off).to(dev)

        records, box_off = scene_only(boxes7)
        cut = None
        if cut_boxes is not None and len(cut_boxes):
            cut = scene_only(cut_boxes) + (a["cut_from"], a["cut_to"])
        counts, _, rows = S.rows_in_boxes_exact(a["points"], a["batch_offsets"], B, records, box_off, cut=cut, capacity=self.capacity)
        return counts, rows


class NuScenesSweepLoader:
    """The file side of a NuScenesDataset: root_path and infos as the dataset holds them (info['lidar_path'], info['sweeps'][k]
    = {'lidar_path', 'transform_matrix' (4, 4) f64 or None, 'time_lag'}).  A NuScenesDataset subclass keeps one and hands
    load_raw(index, max_sweeps) to its collate, where the reference calls get_lidar_with_sweeps(index, max_sweeps)."""

    def __init__(self, root_path, infos, center_radius=1.0):
        self.root_path = root_path
        self.infos = infos
        self.center_radius = center_radius

    def read(self, lidar_path):
        return np.fromfile(os.path.join(str(self.root_path), str(lidar_path)), dtype=np.float32, count=-1).reshape([-1, 5])

    def draw(self, info, max_sweeps):
        """the reference's draw, from numpy's global stream (the augmentor draws from it next)"""
        return np.random.choice(len(info['sweeps']), max_sweeps - 1, replace=False)

    def get_sweep(self, sweep_info):
        return get_sweep(self.read(sweep_info['lidar_path']), sweep_info['transform_matrix'], sweep_info['time_lag'],
                         self.center_radius)

    def get_lidar_with_sweeps(self, index, max_sweeps=1):
        info = self.infos[index]
        key = self.read(info['lidar_path'])
        drawn = [info['sweeps'][k] for k in self.draw(info, max_sweeps)]
        return get_lidar_with_sweeps(key, [(self.read(s['lidar_path']), s['transform_matrix'], s['time_lag']) for s in drawn],
                                     self.center_radius)

    def load_raw(self, index, max_sweeps=1):
        """The same draw as get_lidar_with_sweeps, nothing computed: the scene for pack_sweeps."""
        info = self.infos[index]
        scene = [(self.read(info['lidar_path']), None, 0.0, True)]
        for k in self.draw(info, max_sweeps):
            s = info['sweeps'][k]
            scene.append((self.read(s['lidar_path']), s['transform_matrix'], s['time_lag'], False))
        return scene
