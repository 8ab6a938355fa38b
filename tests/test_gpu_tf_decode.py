"""The device box decode of TransFusionHead (fnp_tf_decode: get_bboxes + decode_bbox(filter=True)) against the reference's own
output, tests/golden/proposals_golden.npz.  Exact: centre, height, velocity, labels (the zero-score rule and the relabel table
included), the keep mask, the counts and the query order.  Scores, sizes and yaw: against the f64 values of the fixture, inside
twice the reference's own f32-against-f64 error on the same inputs (the fixture's `<case>_err_ulp`); the case generator has
asserted that no keep decision lies within that allowance of its threshold."""
import os

import numpy as np
import pytest
import torch

import ref_proposals as RP

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proposals_golden.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def make(name):
    from findnpropagate_amd.dense_heads.transfusion_proposals import BoxDecoder

    c = RP.DECODE_CASES[name]
    return BoxDecoder(RP.decode_post_cfg(c), RP.DECODE_STRIDE, RP.DECODE_VOXEL, RP.DECODE_PCR, RP.DECODE_C, c["unknown_labels"], c["relabel"])


def inputs(name, dev):
    p, labels = RP.decode_inputs(name)
    return {k: torch.from_numpy(v).to(dev) for k, v in p.items()}, torch.from_numpy(labels).to(dev), p, labels


@pytest.mark.parametrize("name", list(RP.DECODE_CASES))
def test_decode_equals_reference(cuda, gold, name):
    c = RP.DECODE_CASES[name]
    preds, labels, p, _ = inputs(name, cuda)
    boxes, scores, out_labels, counts = (t.cpu().numpy() for t in make(name).decode_padded(preds, labels))
    assert np.array_equal(preds["center"].cpu().numpy(), p["center"]), "the inputs are left alone"
    ncol = 9 if c["vel"] else 7
    assert boxes.shape == (c["B"], c["K"], ncol) and out_labels.dtype == np.int32 and counts.dtype == np.int32
    assert np.array_equal(counts, gold[name + "_counts"])
    for b, n in enumerate(counts):                                   # the rows behind the count: all written, all zero
        assert not boxes[b, n:].any() and not scores[b, n:].any() and not out_labels[b, n:].any()
    kb = np.concatenate([boxes[b, :n] for b, n in enumerate(counts)])
    ks = np.concatenate([scores[b, :n] for b, n in enumerate(counts)])
    kl = np.concatenate([out_labels[b, :n] for b, n in enumerate(counts)])
    exact = [0, 1, 2] + ([7, 8] if c["vel"] else [])
    assert np.array_equal(kb[:, exact], gold[name + "_boxes"][:, exact]), "centre, height and velocity: bit for bit, in query order"
    assert np.array_equal(kl, gold[name + "_labels"])
    err = gold[name + "_err_ulp"]
    got = [RP.ulps(ks, gold[name + "_scores64"]).max(), RP.ulps(kb[:, 3:6], gold[name + "_boxes64"][:, 3:6]).max(),
           RP.ulps(kb[:, 6], gold[name + "_boxes64"][:, 6]).max()]
    print(name, "score, size, yaw ulp against f64:", [round(float(g), 3) for g in got], "allowed", (2 * err).round(3).tolist())
    assert got[0] <= 2 * err[0] and got[1] <= 2 * err[1] and got[2] <= 2 * err[2]


def test_zero_score_queries_and_range_limits(cuda):
    """every query, kept or not, through a threshold below zero: labels of zero-score queries are 0 (+ 1), and the two queries
    exactly on the inclusive POST_CENTER_RANGE limits are kept"""
    from findnpropagate_amd.dense_heads.transfusion_proposals import BoxDecoder

    name = "dec_b3_unk"
    c = RP.DECODE_CASES[name]
    preds, labels, p, lab = inputs(name, cuda)
    post = dict(RP.decode_post_cfg(c), SCORE_THRESH=-1.0, SCORE_THRESH_UNK=-1.0, POST_CENTER_RANGE=[-1e9, -1e9, -1e9, 1e9, 1e9, 1e9])
    boxes, scores, out_labels, counts = (t.cpu().numpy() for t in BoxDecoder(post, RP.DECODE_STRIDE, RP.DECODE_VOXEL, RP.DECODE_PCR,
                                                                             RP.DECODE_C).decode_padded(preds, labels))
    assert counts.tolist() == [c["K"]] * c["B"]
    want_boxes, v, want_labels, keep, _ = RP.decode(p, lab, dict(c, thresh_unk=None, unknown_labels=()))
    assert np.array_equal(out_labels, want_labels) and (out_labels[:, 9::10] == 1).all() and (scores[:, 9::10] == 0).all()
    assert np.array_equal(boxes[..., [0, 1, 2, 7, 8]], want_boxes[..., [0, 1, 2, 7, 8]].astype(np.float32))
    assert keep[:, :2].all()
    d = make(name).get_bboxes(preds, labels)
    for b in range(c["B"]):                                          # queries 0 and 1 come first among the kept, in order
        assert np.array_equal(d[b]["pred_boxes"][:2, :3].cpu().numpy(), want_boxes[b, :2, :3].astype(np.float32))
        assert d[b]["pred_boxes"][0, 1].item() == -60.0 and d[b]["pred_boxes"][1, 1].item() == 60.0
        assert d[b]["pred_boxes"][0, 2].item() == -10.0 and d[b]["pred_boxes"][1, 2].item() == 10.0


def test_get_bboxes_lists_and_empty_batch(cuda, gold):
    name = "dec_b3_novel"
    preds, labels, _, _ = inputs(name, cuda)
    dec = make(name)
    out = dec.get_bboxes(preds, labels)
    assert [d["pred_boxes"].shape[0] for d in out] == gold[name + "_counts"].tolist()
    assert all(d["pred_boxes"].shape[1] == 7 and d["pred_labels"].dtype == torch.int32 for d in out)
    assert np.array_equal(np.concatenate([d["pred_labels"].cpu().numpy() for d in out]), gold[name + "_labels"])
    a = dec.decode_padded(preds, labels)
    b = dec.decode_padded(preds, labels)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "run to run"
    empty = {k: v[:0] for k, v in preds.items()}
    boxes, scores, out_labels, counts = dec.decode_padded(empty, labels[:0])
    assert boxes.shape == (0, 200, 7) and counts.shape == (0,) and dec.get_bboxes(empty, labels[:0]) == []
