"""sparse.assemble_sweeps with a window (fnp_assemble_sweeps_window): finished-row sweeps (FNP_SWEEP_FINISHED) in front of and
behind a scene's sweeps, and the cut window (cut_from, cut_to) counted on the card.

Every comparison is bit for bit against numpy (sweeps_scenario.host_vectorised, extended here by the finished rows and the
window) or against the host cut on the host assembly; the plain entry on the same scenes without finished sweeps must give what
it gave before."""
import numpy as np
import pytest
import torch

import sweeps_scenario as SC
from findnpropagate_amd import sparse as S
from findnpropagate_amd import synthetic as syn
from findnpropagate_amd.augmentor import data_augmentor as DA
from findnpropagate_amd.augmentor import database_sampler as DS
from findnpropagate_amd.datasets import nuscenes_sweeps as NS
from test_gpu_gt_sampling import BIG, sampled_boxes
from test_gpu_prepare_points import check_prepared
from test_gpu_sweeps import key, sweep, upload

pytestmark = pytest.mark.gpu


def host_window(raw, sweep_off, scene_sweeps, xform, flags, lag, window, radius=1.0):
    """SC.host_vectorised with finished sweeps (rows taken as they are, all five columns) and the window: -> (points, offsets,
    cut_from, cut_to)"""
    fin = (flags & NS.FINISHED) != 0
    pts, off = SC.host_vectorised(raw, sweep_off, scene_sweeps, xform, np.where(fin, 0, flags), lag, radius)
    counts = []
    for t in range(flags.shape[0]):
        p = raw[sweep_off[t]:sweep_off[t + 1]]
        if flags[t] & SC.DROP_EGO and not fin[t]:
            p = p[~((np.abs(p[:, 0]) < radius) & (np.abs(p[:, 1]) < radius))]
        counts.append(p.shape[0])
    cum = np.concatenate([[0], np.cumsum(counts)])
    for t in np.nonzero(fin)[0]:
        pts[cum[t]:cum[t + 1]] = raw[sweep_off[t]:sweep_off[t + 1]]
    w = np.clip(window, scene_sweeps[:-1, None], scene_sweeps[1:, None])
    return pts, off, (cum[w[:, 0]] - off[:-1]).astype(np.int32), (cum[w[:, 1]] - off[:-1]).astype(np.int32)


def run_window(packed, dev, **kw):
    t = upload(packed, dev)
    return S.assemble_sweeps(*t[:6], packed[6].shape[0], window=t[6], **kw)


def check_window(res, packed):
    pts, off, lo, hi = host_window(*packed)
    n = int(off[-1])
    got = res["points"].cpu().numpy()
    assert np.array_equal(res["batch_offsets"].cpu().numpy(), off) and int(res["n"].item()) == n
    assert np.array_equal(got[:n].view(np.uint32), np.ascontiguousarray(pts).view(np.uint32))
    assert np.all(got[n:] == S.PREP_PAD)
    assert np.array_equal(res["cut_from"].cpu().numpy(), lo) and np.array_equal(res["cut_to"].cpu().numpy(), hi)
    assert np.array_equal(res["window"].cpu().numpy(), np.stack([lo, hi], 1))
    return lo, hi


def finished(rng, n):
    p = rng.uniform(-30, 30, (n, 5)).astype(np.float32)
    p[::3, 0:2] = rng.uniform(-0.9, 0.9, (p[::3].shape[0], 2))          # finished rows inside the ego square stay
    p[:, 4] = rng.uniform(0, 0.5, n)
    return p


def border_batch():
    """scene 0 puts its borders at batch rows 63, 64, 65, 255, 256, 257 (lead | key | sweep | sweep | sweep | tail); scene 1 has
    an empty lead and a first sweep wholly inside the ego square; scene 2 keeps nothing (and has an empty tail); scene 3 carries
    -0.0 and NaN in column 4 of its finished rows"""
    rng = np.random.default_rng(404)
    a = [key(rng, 1), sweep(rng, 1, 1), sweep(rng, 190, 2, matrix=False), sweep(rng, 1, 3)]
    b = [sweep(rng, 70, 1, inside=True), key(rng, 300), sweep(rng, 257, 2)]
    c = [key(rng, 0), sweep(rng, 90, 1, inside=True)]
    d = [key(rng, 700), sweep(rng, 600, 1), sweep(rng, 0, 2), sweep(rng, 511, 3, matrix=False)]
    lead = [finished(rng, 63), finished(rng, 0), None, finished(rng, 130)]
    tail = [finished(rng, 1), finished(rng, 65), finished(rng, 0), finished(rng, 77)]
    lead[3][5:40:5, 4] = -0.0
    lead[3][7:40:5, 4] = np.nan
    tail[3][::4, 4] = np.nan
    tail[3][1::4, 4] = -0.0
    return [a, b, c, d], lead, tail


def test_finished_rows_and_window_match_numpy(cuda):
    scenes, lead, tail = border_batch()
    packed = NS.pack_sweeps(scenes, lead=lead, tail=tail)
    off = packed[1]
    assert all(v in off for v in (63, 64, 65, 255, 256, 257)) and 2000 < off[-1] < 3500
    res = run_window(packed, cuda)
    lo, hi = check_window(res, packed)
    assert lo.tolist() == [63, 0, 0, 130] and hi[2] == 0
    assert hi[1] - lo[1] <= 300 + 257                              # the all-ego sweep at the window's start left nothing
    got = res["points"].cpu().numpy()
    o = res["batch_offsets"].cpu().numpy()
    assert np.array_equal(got[o[3]:o[3] + 130].view(np.uint32), lead[3].view(np.uint32))
    assert np.isnan(got[o[3]:o[3] + 130, 4]).sum() == np.isnan(lead[3][:, 4]).sum() > 0
    # only lead, only tail, neither: the window moves, the rows stay
    for kw in (dict(lead=lead), dict(tail=tail), dict(lead=[None] * 4)):
        p = NS.pack_sweeps(scenes, **kw)
        check_window(run_window(p, cuda), p)
    # the plain entry on the same scenes without finished sweeps: what it gave before, and what the window entry gives
    plain = NS.pack_sweeps(scenes)
    old = S.assemble_sweeps(*upload(plain, cuda), 4)
    want, want_off = SC.host_vectorised(*plain)
    n = int(want_off[-1])
    assert np.array_equal(old["batch_offsets"].cpu().numpy(), want_off)
    assert np.array_equal(old["points"].cpu().numpy()[:n].view(np.uint32), want.view(np.uint32))
    assert "cut_from" not in old
    new = run_window(NS.pack_sweeps(scenes, lead=[None] * 4), cuda)
    assert torch.equal(new["points"].view(torch.int32), old["points"].view(torch.int32))
    assert torch.equal(new["batch_offsets"], old["batch_offsets"])
    # a window that is clamped into the scene, an empty window, no rows at all
    p = list(NS.pack_sweeps(scenes, lead=lead, tail=tail))
    p[6] = np.array([[-5, 99], [3, 3], [9, 2], [p[2][3] + 2, p[2][3] + 3]], np.int32)
    check_window(run_window(p, cuda), p)
    empty = NS.pack_sweeps([[key(np.random.default_rng(0), 0)]], lead=[np.zeros((0, 5), np.float32)])
    res = run_window(empty, cuda)
    assert res["batch_offsets"].cpu().tolist() == [0, 0] and res["window"].cpu().tolist() == [[0, 0]]


def chain(scenes, lead, tail, boxes, dev):
    packed = NS.pack_sweeps(scenes, lead=lead, tail=tail)
    res = run_window(packed, dev)
    check_window(res, packed)
    rec, box_off = (torch.from_numpy(a).to(dev) for a in DA.stack_cut_boxes(boxes, [0] * len(scenes))[:2])
    out = S.prepare_points(res["points"], res["batch_offsets"], len(scenes), None, BIG, cut=(rec, box_off, res["cut_from"], res["cut_to"]))
    finals = []
    for s, l, t, b in zip(scenes, lead, tail, boxes):
        rows = NS.assemble_host(s)
        rows = rows[DS.points_outside_boxes(rows, DS.cut_records(b))]
        finals.append(np.concatenate([l, rows, t], 0))
    check_prepared(out, finals, packed[0].shape[0])
    return finals


def inside_rows(rng, boxes, n):
    """n finished rows at the centres of the boxes: a cut over every row would drop them"""
    p = np.zeros((n, 5), np.float32)
    p[:, :3] = boxes[rng.integers(0, boxes.shape[0], n), :3]
    p[:, 3:] = rng.uniform(0, 1, (n, 2))
    return p


def test_chain_small_scenes(cuda):
    rng = np.random.default_rng(405)
    scenes = [[key(rng, 300), sweep(rng, 257, 1), sweep(rng, 64, 2, matrix=False)], [key(rng, 129)],
              [key(rng, 500), sweep(rng, 130, 1, inside=True), sweep(rng, 700, 2)], [key(rng, 63), sweep(rng, 400, 1)]]
    host = [NS.assemble_host(s) for s in scenes]
    boxes = [sampled_boxes(rng, k, h) for k, h in zip((6, 0, 9, 3), host)]
    lead = [inside_rows(rng, boxes[0], 37), np.zeros((0, 5), np.float32), inside_rows(rng, boxes[2], 100), inside_rows(rng, boxes[3], 1)]
    tail = [inside_rows(rng, boxes[0], 50), finished(rng, 9), np.zeros((0, 5), np.float32), inside_rows(rng, boxes[3], 66)]
    finals = chain(scenes, lead, tail, boxes, cuda)
    assert all(f.shape[0] < l.shape[0] + h.shape[0] + t.shape[0] for f, l, h, t, b in zip(finals, lead, host, tail, boxes) if len(b))
    assert np.array_equal(finals[0][:37], lead[0]) and np.array_equal(finals[3][-66:], tail[3])


def test_chain_ten_sweep_scenes(cuda):
    """4 ten-sweep scenes (~300 k raw rows each) with 2 000 lead and 1 500 tail rows inside the cut boxes"""
    rng = np.random.default_rng(406)
    scenes = [syn.make_raw_sweeps(s) for s in range(4)]
    boxes = [sampled_boxes(rng, 39, s[0][0]) for s in scenes]
    lead = [inside_rows(rng, b, 2000) for b in boxes]
    tail = [inside_rows(rng, b, 1500) for b in boxes]
    chain(scenes, lead, tail, boxes, cuda)


def test_window_entry_captures_and_replays(cuda):
    """captured once with out= and replayed over other rows, flags and windows of the same shapes: the eager results"""
    def content(seed, no_matrix, narrow):
        rng = np.random.default_rng(seed)
        a = [key(rng, 300)] + [sweep(rng, n, j + 1, matrix=j != no_matrix) for j, n in enumerate((257, 64, 500, 0, 191))]
        b = [key(rng, 129), sweep(rng, 700, 1)]
        p = list(NS.pack_sweeps([a, b], lead=[finished(rng, 40), finished(rng, 7)], tail=[finished(rng, 3), None]))
        p[6] = p[6] + np.array([[narrow, -narrow], [0, -narrow]], np.int32)
        return p
    first, second, third = content(1, 2, 0), content(2, 0, 1), content(3, 4, 2)
    assert not np.array_equal(first[4], second[4]) and not np.array_equal(second[6], third[6])
    want = []
    for packed in (second, third):
        r = run_window(packed, cuda)
        check_window(r, packed)
        want.append({k: r[k].clone() for k in ("points", "batch_offsets", "cut_from", "cut_to")})
    assert not torch.equal(want[0]["cut_to"], want[1]["cut_to"])
    static = upload(first, cuda)
    out = S.assemble_sweeps(*static[:6], 2, window=static[6])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            S.assemble_sweeps(*static[:6], 2, window=static[6], out=out)
    torch.cuda.current_stream().wait_stream(s)
    for packed, w in zip((second, third), want):
        for dst, src in zip(static, packed):
            dst.copy_(torch.from_numpy(src))
        out["points"].fill_(-1.0)
        for k in ("batch_offsets", "cut_from", "cut_to"):
            out[k].fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["points"].view(torch.int32), w["points"].view(torch.int32))
        assert all(torch.equal(out[k], w[k]) for k in ("batch_offsets", "cut_from", "cut_to"))
