"""The deferred DataAugmentor on raw scenes (data_dict['raw_sweeps'], no 'points') against the host-mode augmentor on the host
assembly of the same scenes, frame by frame over every case of pseudo_augment_scenario, with HostSceneRows as the provider; and
pack_sweeps with lead / tail rows.  No device: lead, window cut and tail are applied on the host (raw_sweeps_scenario)."""
from pathlib import Path

import numpy as np
import pytest

import pseudo_augment_scenario as SC
import raw_sweeps_scenario as RS
import sweeps_scenario as SW
from findnpropagate_amd.augmentor import data_augmentor as DA
from findnpropagate_amd.augmentor import database_sampler as DS
from findnpropagate_amd.datasets import nuscenes_sweeps as NS


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return RS.setup(tmp_path_factory)


@pytest.mark.parametrize("case", list(SC.CASES))
def test_raw_scenes_match_host_mode(world, case):
    root, fr, st, frames, scenes = world
    host, host_queue = RS.run_host(case, *world)
    programmes = RS.run_deferred_points(case, *world)
    np.random.seed(SC.seed_of(case))
    aug = DA.DataAugmentor(Path(root), SC.augmentor_config(case, fr, st), SC.CLASS_NAMES, deferred=True)
    lost = ego = pasted = fed = 0
    for frame, scene, h, prog in zip(frames, scenes, host, programmes):
        d = aug.forward_head(RS.raw_dict(frame, scene))
        assert 'points' not in d
        provider = RS.Recorder(NS.HostSceneRows(scene, lead=d.get(DA.LEAD_ROWS_KEY)))
        d[DA.SCENE_ROWS_KEY] = provider
        d = aug.forward_tail(d)
        assert 'points' not in d and DA.COPY_STATE_KEY not in d
        assert RS.same_state(np.random.get_state(), h['state'])
        assert np.array_equal(d['gt_boxes'], h['gt_boxes'])
        got, want = d.get(DA.PROGRAM_KEY), prog
        assert (got is None and want is None) or np.array_equal(got, want)
        final = RS.final_rows_host(d, scene)
        assert np.array_equal(final.view(np.uint32), h['points'].view(np.uint32))
        n_lead, n_tail = d.get(DA.LEAD_ROWS_KEY, np.zeros((0, 5))).shape[0], d[DA.TAIL_ROWS_KEY].shape[0]
        lost += int(final.shape[0] - n_lead - n_tail < h['n_in'])
        ego += int(h['n_in'] < RS.raw_rows(scene))
        pasted += int(n_tail > 0)
        fed += int(any(c.sum() > 0 for c in provider.counts))
    assert RS.same_queue(RS.queue_rows(aug), host_queue)
    if SC.CASES[case][0] is not None:
        assert lost > 0, "no frame loses scene rows to gt_sampling's cut"
    assert ego > 0, "no frame drops ego returns inside the window"
    assert pasted > 0, "no frame pastes rows"
    assert fed > 0, "no frame feeds the queue"


def test_forward_without_a_provider_uses_the_host_assembly(world):
    """forward() alone (a worker without a device): HostSceneRows is the default provider"""
    root, fr, st, frames, scenes = world
    case = "shipped"
    host, _ = RS.run_host(case, *world)
    np.random.seed(SC.seed_of(case))
    aug = DA.DataAugmentor(Path(root), SC.augmentor_config(case, fr, st), SC.CLASS_NAMES, deferred=True)
    for frame, scene, h in zip(frames, scenes, host):
        d = aug.forward(RS.raw_dict(frame, scene))
        assert np.array_equal(RS.final_rows_host(d, scene).view(np.uint32), h['points'].view(np.uint32))


def test_world_ops_first_still_raise(world):
    root, fr, st, frames, scenes = world
    cfg = SC.augmentor_config("shipped", fr, st)
    ops = cfg['AUG_CONFIG_LIST']
    cfg['AUG_CONFIG_LIST'] = ops[-4:] + ops[:-4]
    aug = DA.DataAugmentor(Path(root), cfg, SC.CLASS_NAMES, deferred=True)
    with pytest.raises(ValueError):
        aug.forward(RS.raw_dict(frames[0], scenes[0]))
    cfg['AUG_CONFIG_LIST'] = ops[1:3] + ops[-4:] + ops[3:4]
    aug = DA.DataAugmentor(Path(root), cfg, SC.CLASS_NAMES, deferred=True)
    with pytest.raises(ValueError):
        aug.forward(RS.raw_dict(frames[0], scenes[0]))


def _scenes():
    infos, files = SW.make_dataset()
    return [SW.scene_of(infos, files, s, range(len(infos[s]["sweeps"]))) for s in range(SW.NUM_SCENES)]


def test_pack_sweeps_lead_tail_window():
    scenes = _scenes()
    rng = np.random.default_rng(1)
    rows = lambda n: rng.uniform(-5, 5, (n, 5)).astype(np.float32)
    lead = [rows(7), None, rows(0), rows(3)]
    tail = [None, rows(4), rows(2), None]
    plain = NS.pack_sweeps(scenes)
    assert len(plain) == 6
    packed = NS.pack_sweeps(scenes, lead=lead, tail=tail)
    assert len(packed) == 7
    raw, off, scene_sweeps, xform, flags, lag, window = packed
    assert window.dtype == np.int32 and window.shape == (4, 2)
    t = 0
    for b, scene in enumerate(scenes):
        assert scene_sweeps[b] == t
        if lead[b] is not None:
            assert flags[t] == NS.FINISHED and np.array_equal(raw[off[t]:off[t + 1]], lead[b])
            t += 1
        assert window[b, 0] == t and window[b, 1] == t + len(scene)
        for k, (r, m, l, is_key) in enumerate(scene):
            assert np.array_equal(raw[off[t + k]:off[t + k + 1]], r) and not flags[t + k] & NS.FINISHED
        t += len(scene)
        if tail[b] is not None:
            assert flags[t] == NS.FINISHED and np.array_equal(raw[off[t]:off[t + 1]], tail[b])
            t += 1
    assert scene_sweeps[-1] == t == flags.shape[0] and off[-1] == raw.shape[0]
    # without the finished sweeps: the six arrays of the plain call
    own = np.concatenate([np.arange(w0, w1) for w0, w1 in window])
    assert np.array_equal(flags[own], plain[4]) and np.array_equal(lag[own], plain[5]) and np.array_equal(xform[own], plain[3])
    assert np.array_equal(np.concatenate([raw[off[t]:off[t + 1]] for t in own]), plain[0])
    only_lead = NS.pack_sweeps(scenes, lead=[None] * 4)
    assert len(only_lead) == 7 and all(np.array_equal(a, b) for a, b in zip(only_lead[:6], plain))
    assert np.array_equal(only_lead[6], np.stack([plain[2][:-1], plain[2][1:]], 1))


def test_finished_excludes_drop_ego_and_transform():
    NS.check_flags(np.array([0, NS.DROP_EGO, NS.DROP_EGO | NS.TRANSFORM, NS.FINISHED], np.int32))
    for bad in (NS.FINISHED | NS.DROP_EGO, NS.FINISHED | NS.TRANSFORM):
        with pytest.raises(AssertionError):
            NS.check_flags(np.array([0, bad], np.int32))
