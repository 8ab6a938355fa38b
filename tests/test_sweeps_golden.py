"""Multi-sweep assembly on the host (findnpropagate_amd/datasets/nuscenes_sweeps.py) against the REFERENCE's recorded output
(tests/golden/sweeps_golden.npz: NuScenesDataset.get_sweep / get_lidar_with_sweeps run on the samples of sweeps_scenario.py), bit
for bit and with the reference's draw; pack_sweeps' arrays; the host-only workspace query of fnp_assemble_sweeps."""
import os

import numpy as np
import pytest

import sweeps_scenario as SC
from findnpropagate_amd import lib, synthetic as syn
from findnpropagate_amd.datasets import nuscenes_sweeps as NS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweeps_golden.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def dataset():
    return SC.make_dataset()


@pytest.fixture(scope="module")
def loader(dataset, tmp_path_factory):
    infos, files = dataset
    root = tmp_path_factory.mktemp("nuscenes")
    SC.write_files(root, files)
    return NS.NuScenesSweepLoader(root, infos)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                                        b.view(np.uint32) if b.dtype == np.float32 else b)


def test_host_restatement_reproduces_the_reference(golden, dataset):
    infos, files = dataset
    for s in range(SC.NUM_SCENES):
        scene = SC.scene_of(infos, files, s, golden[f"order/{s}"])
        got = NS.get_lidar_with_sweeps(scene[0][0], [t[:3] for t in scene[1:]])
        assert same(got, golden[f"points/{s}"]), s
        assert same(NS.assemble_host(scene), golden[f"points/{s}"]), s
    assert golden["order/2"].size == 0 and golden["points/2"].shape[0] == files[infos[2]["lidar_path"]].shape[0]


def test_get_sweep_reproduces_the_reference(golden, dataset, loader):
    infos, files = dataset
    kept = []
    for k, sw in enumerate(infos[3]["sweeps"]):
        for pts, times in (NS.get_sweep(files[sw["lidar_path"]], sw["transform_matrix"], sw["time_lag"]), loader.get_sweep(sw)):
            assert same(np.ascontiguousarray(pts), golden[f"sweep/3/{k}/points"]), k
            assert same(np.ascontiguousarray(times), golden[f"sweep/3/{k}/times"]), k
        kept.append(pts.shape[0])
    assert kept[1] == 0 and kept[2] == 0 and kept[0] > 0 and kept[3] > 0      # the all-ego and the empty sweep
    # transform_matrix None leaves the sweep's bits alone: the -0.0 coordinates keep their sign
    p0 = golden["sweep/3/0/points"]
    assert np.signbit(p0[p0[:, 2] == 0, 2]).all() and (p0[:, 2] == 0).sum() > 0


def test_loader_draws_what_the_reference_draws(golden, dataset, loader):
    infos, files = dataset
    for s in range(SC.NUM_SCENES):
        np.random.seed(SC.seed_of(s))
        got = loader.get_lidar_with_sweeps(s, max_sweeps=SC.MAX_SWEEPS[s])
        after_host = np.random.random()
        assert same(got, golden[f"points/{s}"]), s
        np.random.seed(SC.seed_of(s))
        scene = loader.load_raw(s, max_sweeps=SC.MAX_SWEEPS[s])
        assert np.random.random() == after_host                       # the same draw: the global stream stays aligned
        want = SC.scene_of(infos, files, s, golden[f"order/{s}"])
        assert len(scene) == len(want) == SC.MAX_SWEEPS[s]
        for a, b in zip(scene, want):
            assert same(a[0], b[0]) and a[2] == b[2] and a[3] == b[3]
            assert (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1]))
        assert same(NS.assemble_host(scene), golden[f"points/{s}"]), s
    with pytest.raises(ValueError):
        loader.load_raw(3, max_sweeps=6)                              # more sweeps than the sample has: the reference's error


def test_pack_sweeps_offsets_and_flags(golden, dataset):
    infos, files = dataset
    scenes = [SC.scene_of(infos, files, s, golden[f"order/{s}"]) for s in range(SC.NUM_SCENES)]
    raw, sweep_off, scene_sweeps, xform, flags, lag = NS.pack_sweeps(scenes)
    T = sum(SC.MAX_SWEEPS)
    assert raw.dtype == np.float32 and raw.shape == (sweep_off[-1], 5) and raw.flags.c_contiguous
    assert sweep_off.dtype == np.int32 and sweep_off.shape == (T + 1,) and sweep_off[0] == 0
    assert scene_sweeps.dtype == np.int32 and scene_sweeps.tolist() == [0, 10, 16, 17, 22]
    assert xform.dtype == np.float64 and xform.shape == (T, 12) and flags.dtype == np.int32 and lag.dtype == np.float32
    t = 0
    for scene in scenes:
        for raw_s, m, time_lag, is_key in scene:
            assert same(raw[sweep_off[t]:sweep_off[t + 1]], raw_s)
            if is_key:
                assert flags[t] == 0 and lag[t] == 0 and not xform[t].any()
            else:
                assert flags[t] == (NS.DROP_EGO | (NS.TRANSFORM if m is not None else 0))
                assert lag[t] == np.float32(time_lag)
                assert np.array_equal(xform[t].reshape(3, 4), m[:3]) if m is not None else not xform[t].any()
            t += 1
    assert [int(f) for f in flags[scene_sweeps[:-1]]] == [0] * 4          # every scene starts with its key frame
    assert (flags == NS.DROP_EGO).sum() == 1                              # the one sweep without a matrix
    assert (NS.DROP_EGO, NS.TRANSFORM) == (lib.FNP_SWEEP_DROP_EGO, lib.FNP_SWEEP_TRANSFORM)
    # no scene at all, and torch tensors on request
    empty = NS.pack_sweeps([[]])
    assert empty[0].shape == (0, 5) and empty[1].tolist() == [0] and empty[2].tolist() == [0, 0]
    import torch
    tens = NS.pack_sweeps(scenes, device="cpu")
    assert [t.dtype for t in tens] == [torch.float32, torch.int32, torch.int32, torch.float64, torch.int32, torch.float32]
    assert np.array_equal(tens[0].numpy(), raw)


def test_vectorised_form_is_the_reference_too(golden, dataset):
    """the large GPU cases are held to vectorised numpy on the packed arrays (sweeps_scenario.host_vectorised); on the fixture
    it gives the reference's recorded bits"""
    infos, files = dataset
    scenes = [SC.scene_of(infos, files, s, golden[f"order/{s}"]) for s in range(SC.NUM_SCENES)]
    want, off = SC.host_vectorised(*NS.pack_sweeps(scenes))
    ref = np.concatenate([golden[f"points/{s}"] for s in range(SC.NUM_SCENES)], 0)
    assert same(want, ref)
    assert off.tolist() == np.concatenate([[0], np.cumsum([golden[f"points/{s}"].shape[0] for s in range(SC.NUM_SCENES)])]).tolist()
    assert (SC.DROP_EGO, SC.TRANSFORM) == (NS.DROP_EGO, NS.TRANSFORM)


def test_fixture_tells_the_fused_accumulation_from_the_unfused(golden, dataset):
    """The recorded transform is numpy's dot, i.e. its BLAS's dgemm, which accumulates fma(m2, z, fma(m1, y, m0*x)) + m3.  The
    product-by-product chain ((m0*x + m1*y) + m2*z) + m3, written out in numpy's elementwise f64 operations, differs from the
    recorded f32 values on the rows built to cancel (sweeps_scenario.cancelling_rows) and nowhere else in that sweep: a device
    kernel that runs the unfused chain cannot pass the fixture test."""
    infos, files = dataset
    sw = infos[3]["sweeps"][3]
    raw, m = files[sw["lidar_path"]], sw["transform_matrix"]
    ego = (np.abs(raw[:, 0]) < 1) & (np.abs(raw[:, 1]) < 1)
    assert not ego[SC.CANCEL_ROWS].any()
    cancel = (np.cumsum(~ego) - 1)[SC.CANCEL_ROWS]                    # where those rows stand behind the ego filter
    p = raw[~ego]
    x, y, z = (p[:, c].astype(np.float64) for c in range(3))
    unfused = np.stack([(((m[c, 0] * x + m[c, 1] * y) + m[c, 2] * z) + m[c, 3]).astype(np.float32) for c in range(3)], 1)
    recorded = golden["sweep/3/3/points"][:, :3]
    differs = (unfused.view(np.uint32) != recorded.view(np.uint32)).any(1)
    assert differs[cancel].sum() >= 1 and differs.sum() == differs[cancel].sum()
    assert np.abs(recorded[cancel, :2]).min(1).max() < 1e-6                                   # they do land on an axis


def test_make_raw_sweeps_is_a_ten_sweep_sample():
    scene = syn.make_raw_sweeps(3)
    assert len(scene) == 10 and scene[0][3] and not any(s[3] for s in scene[1:])
    assert sum(s[1] is None for s in scene[1:]) == 1
    assert all(s[0].dtype == np.float32 and s[0].shape[1] == 5 for s in scene)
    raw_rows = sum(s[0].shape[0] for s in scene)
    out = NS.assemble_host(scene)
    ego = sum(int(((np.abs(s[0][:, 0]) < 1) & (np.abs(s[0][:, 1]) < 1)).sum()) for s in scene[1:])
    assert ego > 0 and out.shape == (raw_rows - ego, 5)
    assert same(scene[2][0], syn.make_raw_sweeps(3)[2][0])                # seeded
    # the sweeps land on the key frame's world: a moved sweep's returns lie within centimetres of returns of the key frame
    m = scene[4][1]
    assert abs(np.linalg.det(m[:3, :3]) - 1) < 1e-12 and abs(m[2, 0]) > 0 and abs(m[2, 0]) < 0.01     # rigid, with a tilt


def test_workspace_query_is_host_only():
    L = lib.load()
    q = L.fnp_assemble_sweeps_workspace_bytes
    sizes = [q(n) for n in (0, 1, 255, 256, 257, 347_000, 44_000_000, 2**31 - 1)]
    assert all(v > 0 for v in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert q(-1) == -1 and q(2**31) == -1                                  # FNP_ERR_ARG
