#!/usr/bin/env python3
"""Golden vectors for the inference side of TransFusionHead around its decoder by RUNNING THE REFERENCE:
pcdet/models/dense_heads/transfusion_head.py, TransFusionHead.predict, get_bboxes, decode_bbox and create_2D_grid called unbound
on a stand-in self, on the CPU.

Stand-ins: shared_conv is the identity, heatmap_head returns the case's map, class_encoding is a real nn.Conv1d with the
case's seeded weights, decoder records its arguments and returns the queries, prediction_head returns zeros.  A case on the
probability path hands predict an object whose .detach().sigmoid() is the case's probabilities (the method applies a sigmoid
to whatever the heatmap head returns).  decode_bbox calls .cuda() on its range tensor: Tensor.cuda is a no-op inside this
script only.

Runs in the build container only (needs the reference).  Output: tests/golden/proposals_golden.npz, OUTPUTS only, and a CRC
of every input (tests/ref_proposals.py regenerates the inputs from their seeds); tests/test_proposals_ref.py holds the
restatement to it."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import ref_proposals as RP  # noqa: E402  (the case tables and the input generators only)
from make_heatmap_golden import AttrDict, load_reference  # noqa: E402


class Probs:
    """what heatmap_head returns on the probability path"""

    def __init__(self, p):
        self.p = p

    def detach(self):
        return self

    def sigmoid(self):
        return self.p


def run_predict(th, name):
    c = RP.CASES[name]
    x = torch.from_numpy(RP.case_map(name))
    B, C, H, W = x.shape
    if name == RP.QUERY_CASE:
        feat, w, bias = (torch.from_numpy(a) for a in RP.query_inputs(name))
    else:
        feat, w, bias = torch.zeros(B, 2, H, W), torch.zeros(2, C, 1), torch.zeros(2)
    enc = torch.nn.Conv1d(C, feat.shape[1], 1)
    with torch.no_grad():
        enc.weight.copy_(w)
        enc.bias.copy_(bias)
    seen = {}

    def decoder(query_feat, lidar_feat_flatten, query_pos, bev_pos):
        seen["query_feat"], seen["query_pos"] = query_feat.detach().clone(), query_pos.clone()
        return query_feat

    s = types.SimpleNamespace()
    s.shared_conv = lambda t: t
    s.heatmap_head = lambda t: x if c["from_logits"] else Probs(x)
    s.class_encoding = enc
    s.decoder = decoder
    s.prediction_head = lambda q: {"center": torch.zeros(B, 2, c["K"])}
    s.bev_pos = th.TransFusionHead.create_2D_grid(None, W, H)
    s.nms_kernel_size, s.num_classes, s.num_proposals = 3, C, c["K"]
    s.dataset_name, s.class_names = c["dataset_name"], c["class_names"]
    with torch.no_grad():
        res = th.TransFusionHead.predict(s, feat, {})
    table = {tuple(r): i for i, r in enumerate(s.bev_pos[0].numpy().tolist())}
    pos = seen["query_pos"].flip(dims=[-1]).numpy()
    top_index = np.array([[table[tuple(r)] for r in scene.tolist()] for scene in pos], np.int64)
    return dict(top_class=s.query_labels.numpy(), top_index=top_index, qhs=res["query_heatmap_score"].numpy(),
                query_feat=seen["query_feat"].numpy(), query_pos=seen["query_pos"].numpy(), bev_pos=s.bev_pos[0].numpy()), x


def run_decode(th, name, dtype):
    c = RP.DECODE_CASES[name]
    p, labels = RP.decode_inputs(name)
    s = types.SimpleNamespace()
    s.model_cfg = AttrDict(POST_PROCESSING=AttrDict(RP.decode_post_cfg(c)))
    s.feature_map_stride, s.voxel_size, s.point_cloud_range = RP.DECODE_STRIDE, list(RP.DECODE_VOXEL), list(RP.DECODE_PCR)
    s.num_classes, s.query_labels = RP.DECODE_C, torch.from_numpy(labels)
    s.training, s.pseudo_nms_thresh = False, None
    if c["unknown_labels"]:
        s.pseudo_processor = types.SimpleNamespace(unknown_labels=list(c["unknown_labels"]))
    s.relabel_classes = c["relabel"] is not None
    if s.relabel_classes:
        s.relabel_map = {i: v for i, v in enumerate(c["relabel"])}
    s.decode_bbox = lambda *a, **k: th.TransFusionHead.decode_bbox(s, *a, **k)
    preds = {k: torch.from_numpy(v).to(dtype).clone() for k, v in p.items()}
    out = th.TransFusionHead.get_bboxes(s, preds)
    return out, p, labels


def main():
    torch.set_num_threads(1)
    th = load_reference()[0]
    torch.Tensor.cuda = lambda self, *a, **k: self          # decode_bbox's range tensor stays on the CPU (this script only)
    save = {}
    for name, c in RP.CASES.items():
        out, x = run_predict(th, name)
        save[name + "_crc"] = np.array([RP.crc(x.numpy())], np.int64)
        keys = ["top_class", "top_index", "qhs"] + (["query_feat", "query_pos", "bev_pos"] if name == RP.QUERY_CASE else [])
        for k in keys:
            save[f"{name}_{k}"] = out[k]
        if name == RP.QUERY_CASE:
            save[name + "_query_crc"] = np.array([RP.crc(a) for a in RP.query_inputs(name)], np.int64)
        print(name, tuple(x.shape), "K", c["K"])
    # the reference's own f32 sigmoid against f64 on the `sigmoid` case's logits
    x = RP.case_map("sigmoid")
    want = 1 / (1 + np.exp(-x.astype(np.float64)))
    err = float(RP.ulps(torch.from_numpy(x).sigmoid().numpy(), want).max())
    gaps = np.diff(np.sort(want.ravel())) / np.spacing(np.sort(want.ravel())[1:].astype(np.float32))
    assert gaps.min() >= 780, gaps.min()
    save["sigmoid_ref_ulp"] = np.array([err])
    print("reference f32 sigmoid against f64:", err, "ulp; smallest gap of neighbours", float(gaps.min()), "ulp")
    for name, c in RP.DECODE_CASES.items():
        o32, p, labels = run_decode(th, name, torch.float32)
        o64, _, _ = run_decode(th, name, torch.float64)
        counts = np.array([d["pred_boxes"].shape[0] for d in o32], np.int32)
        assert counts.tolist() == [d["pred_boxes"].shape[0] for d in o64], "the f32 and the f64 run keep different queries"
        b32 = np.concatenate([d["pred_boxes"].numpy() for d in o32])
        b64 = np.concatenate([d["pred_boxes"].numpy() for d in o64])
        s32 = np.concatenate([d["pred_scores"].numpy() for d in o32])
        s64 = np.concatenate([d["pred_scores"].numpy() for d in o64])
        l32 = np.concatenate([d["pred_labels"].numpy() for d in o32]).astype(np.int32)
        assert np.array_equal(l32, np.concatenate([d["pred_labels"].numpy() for d in o64]))
        err = np.array([RP.ulps(s32, s64).max(), RP.ulps(b32[:, 3:6], b64[:, 3:6]).max(), RP.ulps(b32[:, 6], b64[:, 6]).max()])
        # decision margins: no f64 score of ANY query within the allowance of its threshold, no centre on a range limit but
        # the two queries placed there
        boxes, v, _, keep, thresh = RP.decode(p, labels, c)
        assert np.array_equal(keep.sum(1).astype(np.int32), counts), "the restatement keeps different queries"
        margin = np.abs(v - thresh.astype(np.float64)) / np.spacing(thresh).astype(np.float64)
        assert margin.min() > 2 * err[0] + 1, margin.min()
        lim = np.asarray(RP.DECODE_POST["POST_CENTER_RANGE"], np.float32)
        on_limit = (boxes[..., :3].astype(np.float32) == lim[:3]) | (boxes[..., :3].astype(np.float32) == lim[3:])
        assert not on_limit[:, 2:].any() and on_limit[:, :2, 1:].all() and not on_limit[:, :2, 0].any()
        assert keep[:, :2].all()
        save.update({name + "_boxes": b32, name + "_scores": s32, name + "_labels": l32, name + "_counts": counts,
                     name + "_boxes64": b64, name + "_scores64": s64, name + "_err_ulp": err,
                     name + "_crc": np.array([RP.crc(p[k]) for k in sorted(p)] + [RP.crc(labels)], np.int64)})
        print(name, "kept", counts.tolist(), "reference f32 against f64 (score, size, yaw) ulp:", err.tolist())
    path = os.path.join(HERE, "proposals_golden.npz")
    np.savez_compressed(path, **save)
    print(len(save), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
