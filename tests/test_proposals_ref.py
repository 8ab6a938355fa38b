"""tests/ref_proposals.py (the CPU restatement of TransFusionHead's proposals, query initialisation and box decode) and the
plain-torch mirrors of dense_heads.transfusion_proposals against the reference's own output, tests/golden/proposals_golden.npz;
and the Python wrappers' host-side argument checks, which must fail before the library is loaded.  No GPU."""
import os

import numpy as np
import pytest
import torch

import ref_proposals as RP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proposals_golden.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def restated():
    return {name: RP.proposals(RP.case_map(name), c) for name, c in RP.CASES.items()}


def fixture_scores(gold, name):
    """top_score of the fixture: query_heatmap_score at the query's own class"""
    return np.take_along_axis(gold[name + "_qhs"], gold[name + "_top_class"][:, None, :], axis=1)[:, 0]


@pytest.mark.parametrize("name", list(RP.CASES))
def test_inputs_regenerate(gold, name):
    assert RP.crc(RP.case_map(name)) == int(gold[name + "_crc"][0])


@pytest.mark.parametrize("name", [n for n, c in RP.CASES.items() if c["exact"]])
def test_restatement_equals_reference(gold, restated, name):
    top_class, top_index, top_score, qhs = restated[name]
    assert (top_score > 0).all() and all(np.unique(s).size == s.size for s in top_score), "the case is meant to have no ties"
    assert np.array_equal(top_class, gold[name + "_top_class"])
    assert np.array_equal(top_index, gold[name + "_top_index"])
    assert np.array_equal(qhs, gold[name + "_qhs"])
    assert np.array_equal(top_score, fixture_scores(gold, name))


@pytest.mark.parametrize("name", [n for n, c in RP.CASES.items() if not c["exact"]])
def test_tied_cases_agree_where_the_reference_is_defined(gold, restated, name):
    """the value sequences are equal; classes and indices are equal up to the first tied (or zero) value of a scene"""
    c = RP.CASES[name]
    top_class, top_index, top_score, _ = restated[name]
    want = fixture_scores(gold, name)
    assert np.array_equal(top_score, want)
    HW = c["H"] * c["W"]
    for b in range(c["B"]):
        s = top_score[b]
        tied = np.nonzero((s[1:] == s[:-1]) | (s[1:] == 0))[0]
        first = int(tied[0]) if tied.size else s.size
        if s[0] == 0:
            first = 0
        assert np.array_equal(top_class[b, :first], gold[name + "_top_class"][b, :first])
        assert np.array_equal(top_index[b, :first], gold[name + "_top_index"][b, :first])
        flat = top_class[b] * HW + top_index[b]
        assert np.unique(flat).size == flat.size
        order = np.lexsort((flat, -s.astype(np.float64)))
        assert np.array_equal(order, np.arange(s.size)), "value descending, then flat index ascending"
        zero = flat[s == 0]
        if zero.size:                                              # the fill: the lowest indices that are no positive cell
            free = np.setdiff1d(np.arange(c["K"]), flat[s > 0])
            assert np.array_equal(zero, free[:zero.size])


def test_tied_cases_do_have_ties(restated):
    assert any((s[1:] == s[:-1]).any() for s in restated["ties"][2])
    assert all(0 < (s > 0).sum() < RP.CASES["zerofill"]["K"] for s in restated["zerofill"][2])
    assert (restated["refine"][2] >= 0.5).all()


def test_border_case(restated):
    top_class, top_index, _, _ = restated["borders"]
    W = RP.CASES["borders"]["W"]
    c, h, w = RP.BORDER_POINT
    assert (top_class[0, 0], top_index[0, 0]) == (c, h * W + w)
    c, h, w = RP.BORDER_ORDINARY
    assert not ((top_class[0] == c) & (top_index[0] == h * W + w)).any()


@pytest.mark.parametrize("name", list(RP.CASES))
def test_plain_mirror_equals_restatement(restated, name):
    from findnpropagate_amd.dense_heads.transfusion_proposals import point_classes, proposals_plain

    c = RP.CASES[name]
    assert point_classes(c["dataset_name"], c["C"], c["class_names"]) == RP.point_classes(c)
    got = proposals_plain(torch.from_numpy(RP.case_map(name)), c["K"], RP.point_classes(c), from_logits=c["from_logits"])
    for g, w in zip(got, restated[name]):
        assert np.array_equal(g.numpy(), w)


def test_query_initialisation(gold):
    from findnpropagate_amd.dense_heads.transfusion_proposals import init_queries_plain

    name = RP.QUERY_CASE
    c = RP.CASES[name]
    feat, w, bias = RP.query_inputs(name)
    assert [RP.crc(a) for a in (feat, w, bias)] == gold[name + "_query_crc"].tolist()
    table = RP.bev_pos_table(c["H"], c["W"])
    assert np.array_equal(table, gold[name + "_bev_pos"])
    flat = feat.reshape(c["B"], RP.QUERY_FEATURES, -1)
    qf, qp = RP.init_queries(flat, table, w[:, :, 0], bias, gold[name + "_top_class"], gold[name + "_top_index"])
    assert np.array_equal(qf, gold[name + "_query_feat"]) and np.array_equal(qp, gold[name + "_query_pos"])
    qf, qp = init_queries_plain(torch.from_numpy(flat), torch.from_numpy(table), torch.from_numpy(w), torch.from_numpy(bias),
                                torch.from_numpy(gold[name + "_top_class"]), torch.from_numpy(gold[name + "_top_index"]))
    assert np.array_equal(qf.numpy(), gold[name + "_query_feat"]) and np.array_equal(qp.numpy(), gold[name + "_query_pos"])


def sigmoid_bound(gold):
    return float(gold["sigmoid_ref_ulp"][0]) + RP.SIGMOID_EXTRA_ULP


def test_sigmoid_case_margins(gold):
    x = RP.case_map("sigmoid").astype(np.float64).ravel()
    s = np.sort(1 / (1 + np.exp(-x)))
    gaps = np.diff(s) / np.spacing(s[1:].astype(np.float32))
    assert gaps.min() >= 780 > 2 * sigmoid_bound(gold)
    assert 1.0 < float(gold["sigmoid_ref_ulp"][0]) < 2.0


def compact(c, boxes, v, labels, keep):
    return boxes[keep], v[keep], labels[keep], keep.sum(1).astype(np.int32)


@pytest.mark.parametrize("name", list(RP.DECODE_CASES))
def test_decode_restatement(gold, name):
    c = RP.DECODE_CASES[name]
    p, labels = RP.decode_inputs(name)
    assert [RP.crc(p[k]) for k in sorted(p)] + [RP.crc(labels)] == gold[name + "_crc"].tolist()
    boxes, v, out_labels, keep, _ = RP.decode(p, labels, c)
    b, s, l, counts = compact(c, boxes, v, out_labels, keep)
    assert np.array_equal(counts, gold[name + "_counts"]) and np.array_equal(l, gold[name + "_labels"])
    assert keep[:, :2].all(), "the two queries on the inclusive range limits are kept"
    assert (out_labels[:, 9::10] == (1 if c["relabel"] is None else c["relabel"][1])).all(), "a zero score column gives label 0 (+ 1)"
    exact = [0, 1, 2] + ([7, 8] if c["vel"] else [])
    assert np.array_equal(b[:, exact].astype(np.float32), gold[name + "_boxes"][:, exact])
    np.testing.assert_allclose(b[:, 3:], gold[name + "_boxes64"][:, 3:], rtol=1e-13, atol=0)   # (its centres are formed in f64)
    np.testing.assert_allclose(s, gold[name + "_scores64"], rtol=1e-13, atol=0)
    err = gold[name + "_err_ulp"]
    assert RP.ulps(gold[name + "_scores"], s).max() <= err[0] + 1e-6
    assert RP.ulps(gold[name + "_boxes"][:, 3:6], b[:, 3:6]).max() <= err[1] + 1e-6
    assert RP.ulps(gold[name + "_boxes"][:, 6], b[:, 6]).max() <= err[2] + 1e-6


@pytest.mark.parametrize("name", list(RP.DECODE_CASES))
def test_decode_plain_mirror(gold, name):
    from findnpropagate_amd.dense_heads.transfusion_proposals import BoxDecoder, get_bboxes_plain

    c = RP.DECODE_CASES[name]
    p, labels = RP.decode_inputs(name)
    dec = BoxDecoder(RP.decode_post_cfg(c), RP.DECODE_STRIDE, RP.DECODE_VOXEL, RP.DECODE_PCR, RP.DECODE_C, c["unknown_labels"], c["relabel"])
    preds = {k: torch.from_numpy(v) for k, v in p.items()}
    out = get_bboxes_plain(preds, torch.from_numpy(labels), dec)
    assert np.array_equal(preds["center"].numpy(), p["center"]), "the mirror leaves its inputs alone"
    assert [d["pred_boxes"].shape[0] for d in out] == gold[name + "_counts"].tolist()
    assert np.array_equal(np.concatenate([d["pred_boxes"].numpy() for d in out]), gold[name + "_boxes"])
    assert np.array_equal(np.concatenate([d["pred_scores"].numpy() for d in out]), gold[name + "_scores"])
    assert np.array_equal(np.concatenate([d["pred_labels"].numpy() for d in out]), gold[name + "_labels"])


# ---- host-side argument checks: they fail before the library is loaded ----------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    from findnpropagate_amd import lib

    def boom():
        raise RuntimeError("the library must not be loaded for a call that fails its argument checks")

    monkeypatch.setattr(lib, "load", boom)


def test_proposals_argument_checks(no_library):
    from findnpropagate_amd.dense_heads.transfusion_proposals import HeatmapProposals

    with pytest.raises(AssertionError, match="NMS_KERNEL_SIZE"):
        HeatmapProposals(200, 1, 10, "nuScenes")
    with pytest.raises(AssertionError, match="num_classes"):
        HeatmapProposals(200, 3, 65, "nuScenes")
    with pytest.raises(AssertionError, match="num_proposals"):
        HeatmapProposals(4096, 3, 10, "nuScenes")
    with pytest.raises(AssertionError, match="class_names"):
        HeatmapProposals(50, 3, 3, "kitti")
    head = HeatmapProposals(200, 3, 10, "nuScenes")
    assert head.point_mask == (1 << 8) | (1 << 9)
    assert HeatmapProposals(50, 3, 3, "Waymo").point_mask == 0b110
    assert HeatmapProposals(50, 3, 4, "kitti", ["Car", "Pedestrian", "Van", "Cyclist"]).point_mask == 0b1010
    with pytest.raises(AssertionError, match="B, C, H, W"):
        head(torch.zeros(10, 8, 8))
    with pytest.raises(AssertionError, match="float32"):
        head(torch.zeros(1, 10, 8, 8, dtype=torch.float16))
    with pytest.raises(AssertionError, match="classes"):
        head(torch.zeros(1, 9, 8, 8))
    with pytest.raises(AssertionError, match="exceeds"):
        head(torch.zeros(1, 10, 4, 4))                              # K = 200 > C*H*W = 160
    with pytest.raises(RuntimeError, match="must not be loaded"):
        head(torch.zeros(1, 10, 8, 8))                              # a valid call does reach the library


def test_init_queries_and_decoder_argument_checks(no_library):
    from findnpropagate_amd.dense_heads.transfusion_proposals import BoxDecoder, HeatmapProposals

    head = HeatmapProposals(4, 3, 10, "nuScenes")
    feat, pos, w, bias = torch.zeros(1, 16, 64), torch.zeros(64, 2), torch.zeros(16, 10, 1), torch.zeros(16)
    cls, idx = torch.zeros(1, 4, dtype=torch.int64), torch.zeros(1, 4, dtype=torch.int64)
    with pytest.raises(AssertionError, match="bev_pos"):
        head.init_queries(feat, torch.zeros(63, 2), w, bias, cls, idx)
    with pytest.raises(AssertionError, match="enc_weight"):
        head.init_queries(feat, pos, torch.zeros(16, 9, 1), bias, cls, idx)
    with pytest.raises(AssertionError, match="int64"):
        head.init_queries(feat, pos, w, bias, cls.int(), idx.int())
    with pytest.raises(AssertionError, match="float32"):
        head.init_queries(feat.double(), pos, w, bias, cls, idx)
    c = RP.DECODE_CASES["dec_b1"]
    dec = BoxDecoder(RP.decode_post_cfg(c), RP.DECODE_STRIDE, RP.DECODE_VOXEL, RP.DECODE_PCR, RP.DECODE_C)
    p, labels = RP.decode_inputs("dec_b1")
    preds = {k: torch.from_numpy(v) for k, v in p.items()}
    with pytest.raises(AssertionError, match="dim"):
        dec.decode_padded({**preds, "dim": preds["dim"][:, :2]}, torch.from_numpy(labels))
    with pytest.raises(AssertionError, match="float32"):
        dec.decode_padded({**preds, "rot": preds["rot"].double()}, torch.from_numpy(labels))
    with pytest.raises(AssertionError, match="query_labels"):
        dec.decode_padded(preds, torch.from_numpy(labels).int())
    with pytest.raises(AssertionError, match="POST_CENTER_RANGE"):
        BoxDecoder({"SCORE_THRESH": 0.1, "POST_CENTER_RANGE": [0, 1, 2]}, 8, [0.1, 0.1], [0, 0], 10)
