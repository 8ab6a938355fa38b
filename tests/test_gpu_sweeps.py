"""sparse.assemble_sweeps (fnp_assemble_sweeps): NuScenesDataset.get_lidar_with_sweeps of a batch on the device.

Every comparison is bit for bit: points[:n] (as 32-bit words, so that the sign of a zero counts), batch_offsets and n against the
reference's recorded output (the fixture scenes) or the host restatement of its arithmetic (datasets.nuscenes_sweeps), and
points[n:] == PREP_PAD.  No tolerance anywhere: the f64 transform rounds to f32 once, and a differing element would mean a wrong
order of operations, not noise (test_chain_to_voxels_matches_oracle holds returns that cancel to 1e-9 m, where the last f64 bit
shows in the f32 result)."""
import os

import numpy as np
import pytest
import torch

import sweeps_scenario as SC
import test_gpu_prepare_points as TP
from findnpropagate_amd import sparse as S
from findnpropagate_amd import synthetic as syn
from findnpropagate_amd.datasets import nuscenes_sweeps as NS

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweeps_golden.npz")
BORDER_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257)


def upload(packed, dev):
    return [torch.from_numpy(a).to(dev) for a in packed]


def check(res, finals, n_rows):
    """finals: the expected (m_b, 5) rows of every scene"""
    off = res["batch_offsets"].cpu().numpy()
    want_off = np.concatenate([[0], np.cumsum([f.shape[0] for f in finals])]).astype(np.int32)
    assert np.array_equal(off, want_off)
    n = int(res["n"].item())
    assert n == want_off[-1]
    got = res["points"].cpu().numpy()
    assert got.shape == (n_rows, 5) and got.dtype == np.float32
    want = np.ascontiguousarray(np.concatenate(finals, 0), dtype=np.float32) if finals else np.zeros((0, 5), np.float32)
    assert np.array_equal(got[:n].view(np.uint32), want.view(np.uint32))
    assert np.all(got[n:] == S.PREP_PAD)


def run(scenes, dev, **kw):
    packed = NS.pack_sweeps(scenes)
    return S.assemble_sweeps(*upload(packed, dev), len(scenes), **kw), packed[0].shape[0]


def run_and_check(scenes, dev, center_radius=1.0):
    res, n_rows = run(scenes, dev, center_radius=center_radius)
    check(res, [NS.assemble_host(s, center_radius) for s in scenes], n_rows)
    return res


def sweep(rng, n, j, matrix=True, inside=False):
    return (SC.rows(rng, n, inside), SC.rigid(rng, j) if matrix else None, 0.05 * j + 1e-3 * rng.random(), False)


def key(rng, n):
    return (SC.rows(rng, n), None, 0.0, True)


def test_fixture_scenes_match_reference(cuda):
    """all fixture scenes in one batch, their sweeps in the order the reference drew: the reference's recorded output"""
    g = np.load(GOLDEN)
    infos, files = SC.make_dataset()
    scenes = [SC.scene_of(infos, files, s, g[f"order/{s}"]) for s in range(SC.NUM_SCENES)]
    res, n_rows = run(scenes, cuda)
    check(res, [g[f"points/{s}"] for s in range(SC.NUM_SCENES)], n_rows)


def border_scenes():
    """sweep lengths through 0, 1, 63, 64, 65, 255, 256, 257 (twice, shifted, so that sweep and scene borders fall inside a wave,
    on a wave edge and on a workgroup edge), an all-dropped sweep, an empty key frame, a scene without rows, a key frame alone"""
    rng = np.random.default_rng(99)
    a = [key(rng, 256)] + [sweep(rng, n, j + 1, matrix=j != 3) for j, n in enumerate(BORDER_LENGTHS)]
    b = [key(rng, 0)] + [sweep(rng, n, j + 1) for j, n in enumerate(BORDER_LENGTHS[::-1])] + [sweep(rng, 130, 9, inside=True)]
    c = [key(rng, 0)]
    d = [key(rng, 191)]
    e = [key(rng, 64), sweep(rng, 64, 1, inside=True), sweep(rng, 257, 2), sweep(rng, 0, 3), sweep(rng, 63, 4)]
    return [a, b, c, d, e]


def test_borders(cuda):
    scenes = border_scenes()
    res = run_and_check(scenes, cuda)
    off = res["batch_offsets"].cpu().numpy()
    assert off[2] == off[3] and off[3] < off[4]
    # the same rows and sweeps as ONE scene (key frames in the middle of it keep flags 0)
    packed = list(NS.pack_sweeps(scenes))
    packed[2] = np.array([0, packed[4].shape[0]], np.int32)
    one = S.assemble_sweeps(*upload(packed, cuda), 1)
    check(one, [np.concatenate([NS.assemble_host(s) for s in scenes], 0)], packed[0].shape[0])
    # no rows at all: no sweep, and sweeps without rows
    for empty in ([[]], [[key(np.random.default_rng(0), 0)], [key(np.random.default_rng(0), 0), sweep(np.random.default_rng(0), 0, 1)]]):
        res, n_rows = run(empty, cuda)
        assert n_rows == 0 and res["points"].shape == (0, 5)
        assert res["batch_offsets"].cpu().tolist() == [0] * (len(empty) + 1) and int(res["n"].item()) == 0


def edge_rows(r):
    """x or y on, just inside and just outside the ego square of radius r, the other coordinate matching (inside) or not; every
    pair of edge values; -0.0 in every coordinate"""
    r = np.float32(r)
    vals = np.array([r, -r, np.nextafter(r, np.float32(0)), -np.nextafter(r, np.float32(0)),
                     np.nextafter(r, np.float32(2) * r), -np.nextafter(r, np.float32(2) * r)], np.float32)
    xy = [(v, o) for v in vals for o in (0.5 * r, -0.25 * r, 1.5 * r, -0.0, 0.0)]
    xy += [(o, v) for v, o in list(xy)]
    xy += [(a, b) for a in vals for b in vals]
    xy += [(-0.0, -0.0), (0.0, -0.0), (-0.0, 3.0 * r), (3.0 * r, -0.0)]
    p = np.zeros((len(xy), 5), np.float32)
    p[:, 0:2] = np.array(xy, np.float32)
    p[:, 2] = np.where(np.arange(len(xy)) % 3 == 0, np.float32(-0.0), np.float32(-1.25))
    p[:, 3] = np.arange(len(xy))
    p[:, 4] = 7
    return p


def test_ego_edge_values(cuda):
    rng = np.random.default_rng(5)
    for radius in (1.0, 2.5):
        p = np.concatenate([edge_rows(1.0), edge_rows(2.5)], 0)
        scene = [(p.copy(), None, 0.0, True), (p.copy(), None, 0.1, False), (p.copy(), SC.rigid(rng, 1), 0.2, False)]
        res = run_and_check([scene], cuda, center_radius=radius)
        got = res["points"].cpu().numpy()
        n = p.shape[0]
        inside = (np.abs(p[:, 0]) < radius) & (np.abs(p[:, 1]) < radius)
        assert 0 < inside.sum() < n and int(res["n"].item()) == 3 * n - 2 * inside.sum()
        assert np.array_equal(got[:n, :4].view(np.uint32), p[:, :4].view(np.uint32))             # key-frame rows inside the square stay
        kept = p[~inside]
        bare = got[n:n + kept.shape[0]]
        assert np.array_equal(bare[:, :4].view(np.uint32), kept[:, :4].view(np.uint32))          # no matrix: the bits are left alone
        assert np.signbit(bare[:, :3][kept[:, :3] == 0]).sum() == np.signbit(kept[:, :3][kept[:, :3] == 0]).sum() > 0
        assert np.all(bare[:, 4] == np.float32(0.1)) and np.all(got[:n, 4] == 0)
        # exactly on the edge is outside (strict comparisons), one step inside is inside
        on = (np.abs(p[:, 0]) == radius) | (np.abs(p[:, 1]) == radius)
        assert on.sum() > 0 and not inside[on].any()


_SCAN = {}


def scan_data():
    """2^21 + 1 raw rows and a layout of 3 scenes with 23 sweeps of uneven lengths over them (built once)"""
    if not _SCAN:
        rng = np.random.default_rng(2021)
        R = (1 << 21) + 1
        raw = np.empty((R, 5), np.float32)
        raw[:, 0:2] = rng.uniform(-30, 30, (R, 2)).astype(np.float32)
        near = rng.random(R) < 0.15
        raw[near, 0:2] *= np.float32(0.05)
        raw[:, 2] = rng.uniform(-3, 2, R)
        raw[:, 3] = rng.uniform(0, 255, R)
        raw[:, 4] = 0
        T = 23
        frac = np.sort(rng.random(T - 1))
        scene_sweeps = np.array([0, 9, 10, T], np.int32)
        flags = np.full(T, NS.DROP_EGO | NS.TRANSFORM, np.int32)
        flags[scene_sweeps[:-1]] = 0
        flags[5] = NS.DROP_EGO
        xform = np.stack([SC.rigid(rng, j)[:3].reshape(12) for j in range(T)])
        lag = (0.05 * np.arange(T) + 1e-3 * rng.random(T)).astype(np.float32)
        lag[scene_sweeps[:-1]] = 0
        _SCAN.update(raw=raw, frac=frac, scene_sweeps=scene_sweeps, flags=flags, xform=xform, lag=lag)
    return _SCAN


@pytest.mark.parametrize("groups,extra", [(4096, 0), (4096, 1), (8192, 0), (8192, 1)])
def test_scan_shapes(cuda, groups, extra):
    """fnp_scan over the counts of the 256-row workgroups changes its launch shape with every 4096 counts (scan.hip: one more
    workgroup of the single-launch scan per tile of kTile = 4096), and at 16 tiles = 65536 counts goes from one launch to three.
    R = groups * 256 rows is the last row count with `groups` workgroups, one row more the first with groups + 1: 4096 | 4097 and
    8192 | 8193 counts, 2^20 (+1) and 2^21 (+1) rows.  Left out, for needing more than 2^21 raw rows: the further tile borders
    12288, 16384, ... 61440 counts (3 M to 15 M rows; the same kernel with one more workgroup each) and the border to the
    three-launch scan at 65536 counts (2^24 rows, 336 MB of raw rows)."""
    d = scan_data()
    R = groups * 256 + extra
    assert (R + 255) // 256 == groups + extra and R <= d["raw"].shape[0]
    raw = d["raw"][:R]
    sweep_off = np.concatenate([[0], np.floor(d["frac"] * R), [R]]).astype(np.int32)
    want, want_off = SC.host_vectorised(raw, sweep_off, d["scene_sweeps"], d["xform"], d["flags"], d["lag"])
    res = S.assemble_sweeps(*upload((raw, sweep_off, d["scene_sweeps"], d["xform"], d["flags"], d["lag"]), cuda), 3)
    n = int(res["n"].item())
    assert 0.9 * R < n < R
    assert np.array_equal(res["batch_offsets"].cpu().numpy(), want_off) and n == want.shape[0]
    got = res["points"].cpu().numpy()
    assert np.array_equal(got[:n].view(np.uint32), want.view(np.uint32))
    assert np.all(got[n:] == S.PREP_PAD)


def test_chain_to_voxels_matches_oracle(cuda, oracle):
    """assemble_sweeps -> prepare_points (recorded program, explicit permutation) -> voxelize, against the host restatement ->
    the host prepare path -> the oracle voxeliser, at 384 x 384 x 40 voxels"""
    scenes = [syn.make_raw_sweeps(5), syn.make_raw_sweeps(6, sweeps=4)]
    assembled = [NS.assemble_host(s) for s in scenes]
    res, n_rows = run(scenes, cuda)
    check(res, assembled, n_rows)
    finals, programs, perms = TP.host_prepare(assembled, [31, 32], TP.TRANSFUSION, TP.SMALL_RANGE)
    prog = torch.from_numpy(TP.DA.stack_programs(programs)).to(cuda)
    perm = torch.from_numpy(np.concatenate(perms)).to(cuda)
    prepared = S.prepare_points(res["points"], res["batch_offsets"], 2, prog, TP.SMALL_RANGE, shuffle=perm)
    TP.check_prepared(prepared, finals, n_rows)
    assert TP._voxelize_check(oracle, prepared, finals, TP.SMALL_RANGE, 160000) > 10000


def test_scene_rows_do_not_depend_on_the_batch(cuda):
    scenes = border_scenes()
    whole, _ = run(scenes, cuda)
    off = whole["batch_offsets"].cpu().numpy()
    got = whole["points"].cpu().numpy()
    for b in (1, 4):
        for batch in ([scenes[b]], [scenes[3], scenes[b], scenes[0]]):
            res, _ = run(batch, cuda)
            o = res["batch_offsets"].cpu().numpy()
            k = len(batch) // 2
            rows = res["points"].cpu().numpy()[o[k]:o[k + 1]]
            assert np.array_equal(rows.view(np.uint32), got[off[b]:off[b + 1]].view(np.uint32))


def test_captures_and_replays_on_one_stream(cuda):
    """captured once with out= and replayed over two other contents of the same shapes: the eager results"""
    def content(seed):
        rng = np.random.default_rng(seed)
        a = [key(rng, 300)] + [sweep(rng, n, j + 1, matrix=j != 2) for j, n in enumerate((257, 64, 500, 0, 191))]
        b = [key(rng, 129), sweep(rng, 700, 1)]
        return NS.pack_sweeps([a, b])
    first, second, third = content(1), content(2), content(3)
    assert all(np.array_equal(first[k], second[k]) for k in (1, 2)) and not np.array_equal(first[0], second[0])
    want = []
    for packed in (second, third):
        r = S.assemble_sweeps(*upload(packed, cuda), 2)
        want.append((r["points"].clone(), r["batch_offsets"].clone()))
    assert not torch.equal(want[0][1], want[1][1])                                   # the kept counts differ too
    static = upload(first, cuda)
    out = S.assemble_sweeps(*static, 2)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            S.assemble_sweeps(*static, 2, out=out)
    torch.cuda.current_stream().wait_stream(s)
    for packed, (pts, off) in zip((second, third), want):
        for dst, src in zip(static, packed):
            dst.copy_(torch.from_numpy(src))
        out["points"].fill_(-1.0)
        out["batch_offsets"].fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["points"].view(torch.int32), pts.view(torch.int32)) and torch.equal(out["batch_offsets"], off)
        assert int(out["n"].item()) == int(off[-1].item())
