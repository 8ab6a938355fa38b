"""Seeded scenario of the sweep-assembly golden (tests/golden/make_sweeps_golden.py, tests/test_sweeps_golden.py,
tests/test_gpu_sweeps.py): four small nuScenes-like samples as a NuScenesDataset holds them, infos plus sweep files.

  scene 0   key frame + 9 sweeps, all drawn (MAX_SWEEPS 10)
  scene 1   key frame + 9 sweeps, 5 of them drawn
  scene 2   a key frame only
  scene 3   key frame + 4 sweeps: one with transform_matrix None (and -0.0 coordinates), one wholly inside the ego square, one
            without rows, one ordinary with 64 rows that the transform brings back onto a key-frame axis (cancelling_rows)
Key frames have ~700 rows, sweeps 0 to ~600.  About a tenth of all rows lie around the ego square, some exactly on its edge."""
import os

import numpy as np

NUM_SCENES = 4
MAX_SWEEPS = (10, 6, 1, 5)
DROP_EGO, TRANSFORM = 1, 2          # the flag bits of fnp_assemble_sweeps


def seed_of(s):
    """seed of the draw in get_lidar_with_sweeps for scene s"""
    return 4200 + s


def rows(rng, n, inside=False):
    p = np.empty((n, 5), np.float32)
    if inside:
        p[:, 0:2] = rng.uniform(-0.999, 0.999, (n, 2))
    else:
        p[:, 0:2] = rng.uniform(-30, 30, (n, 2))
        near = rng.random(n) < 0.1
        p[near, 0:2] = rng.uniform(-1.5, 1.5, (int(near.sum()), 2))
        edge = rng.random(n) < 0.02
        p[edge, 0] = rng.choice(np.array([1.0, -1.0], np.float32), int(edge.sum()))
        p[edge, 1] = rng.uniform(-1.2, 1.2, int(edge.sum()))
    p[:, 2] = rng.uniform(-3, 2, n)
    p[:, 3] = rng.uniform(0, 255, n)
    p[:, 4] = rng.integers(0, 32, n)
    return p


def rigid(rng, j):
    """a rigid transform with small pitch and roll terms, ~0.5 m per sweep"""
    yaw, pitch, roll = rng.normal(0, 0.02), rng.normal(0, 2e-3), rng.normal(0, 2e-3)
    cz, sz, cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    M = np.eye(4)
    M[:3, :3] = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
                 @ np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    M[:3, 3] = [-0.5 * j + rng.normal(0, 0.05), rng.normal(0, 0.05), rng.normal(0, 0.01)]
    return M


CANCEL_ROWS = slice(100, 164)      # rows of scene 3's last sweep that the transform brings back onto a key-frame axis


def cancelling_rows(rng, matrix, n):
    """raw x, y, z = R^T (p - t) of points p ON the key frame's x axis (even rows) or y axis (odd rows), 3 to 30 m out: the
    transform's sum for the other coordinate cancels to ~1e-9 m, where the last bit of the f64 accumulation decides the f32
    result — the rows that tell a fused accumulation (BLAS's dgemm) from a product-by-product one"""
    p = np.zeros((n, 3))
    far = rng.uniform(3, 30, n) * rng.choice([-1.0, 1.0], n)
    p[0::2, 0], p[1::2, 1] = far[0::2], far[1::2]
    p[:, 2] = rng.uniform(-3, 2, n)
    return ((p - matrix[:3, 3]) @ matrix[:3, :3]).astype(np.float32)


def make_dataset():
    """(infos, files): infos as NuScenesDataset.infos, files {relative path: (n, 5) f32} for write_files"""
    rng = np.random.default_rng(20240519)
    infos, files = [], {}
    for s in range(NUM_SCENES):
        key_path = f"samples/LIDAR_TOP/scene{s}_key.pcd.bin"
        files[key_path] = rows(rng, int(rng.integers(650, 750)))
        sweeps = []
        count = (9, 9, 0, 4)[s]
        for k in range(count):
            n, matrix, inside = int(rng.integers(0, 600)), rigid(rng, k + 1), False
            if s == 3:
                n = (300, 150, 0, 420)[k]
                inside = k == 1
                if k == 0:
                    matrix = None
            raw = rows(rng, n, inside)
            if s == 3 and k == 0:
                raw[5:40:5, 0] = -0.0
                raw[7:40:5, 1] = -0.0
                raw[9:40:5, 2] = -0.0
            if s == 3 and k == 3:
                raw[CANCEL_ROWS, :3] = cancelling_rows(rng, matrix, CANCEL_ROWS.stop - CANCEL_ROWS.start)
            path = f"sweeps/LIDAR_TOP/scene{s}_sweep{k}.pcd.bin"
            files[path] = raw
            sweeps.append({"lidar_path": path, "transform_matrix": matrix, "time_lag": 0.05 * (k + 1) + 1e-3 * rng.random()})
        infos.append({"lidar_path": key_path, "sweeps": sweeps})
    return infos, files


def write_files(root, files):
    for path, raw in files.items():
        full = os.path.join(str(root), path)
        os.makedirs(os.path.dirname(full), exist_ok=True)
        raw.tofile(full)


def scene_of(infos, files, s, order):
    """scene s in pack_sweeps' form with its sweeps in `order`"""
    info = infos[s]
    scene = [(files[info["lidar_path"]], None, 0.0, True)]
    for k in order:
        sw = info["sweeps"][int(k)]
        scene.append((files[sw["lidar_path"]], sw["transform_matrix"], sw["time_lag"], False))
    return scene


def host_vectorised(raw, sweep_off, scene_sweeps, xform, flags, lag, radius=1.0):
    """the kernel's contract on packed arrays in vectorised numpy, sweep by sweep: the strict ego test on the f32 values, the
    reference's own expression for the transform (the 4x4 matrix against the f64 stack of x, y, z and ones, stored into f32)"""
    parts, counts = [], []
    for t in range(flags.shape[0]):
        p = raw[sweep_off[t]:sweep_off[t + 1]]
        if flags[t] & DROP_EGO:
            p = p[~((np.abs(p[:, 0]) < radius) & (np.abs(p[:, 1]) < radius))]
        out = np.empty((p.shape[0], 5), np.float32)
        out[:, :4] = p[:, :4]
        if flags[t] & TRANSFORM:
            m = np.vstack((xform[t].reshape(3, 4), [0.0, 0.0, 0.0, 1.0]))
            out[:, :3] = m.dot(np.vstack((p[:, :3].T, np.ones(p.shape[0]))))[:3, :].T
        out[:, 4] = lag[t]
        parts.append(out)
        counts.append(out.shape[0])
    cum = np.concatenate([[0], np.cumsum(counts)])
    return np.concatenate(parts, 0), cum[scene_sweeps].astype(np.int32)
