#!/usr/bin/env python3
"""Golden vectors for TransFusionHead's decoder layer and prediction heads by RUNNING THE REFERENCE:
pcdet/models/model_utils/transfusion_utils.py (PositionEmbeddingLearned, TransformerDecoderLayer) and
pcdet/models/dense_heads/transfusion_head.py (SeparateHead_Transfusion), instantiated through
make_heatmap_golden.load_reference, loaded with the seeded weights of tests/ref_decoder.py, in eval mode, on the CPU in f32.
The attention-alone cases run the layer's own attention class (nn.MultiheadAttention(128, 8)) with identity projections and
zero biases: a product with the identity is exact, so its output is the attention itself.

Runs in the build container only (needs the reference).  Output: tests/golden/decoder_golden.npz: OUTPUTS only, a CRC of every
input, the modules' state_dict keys and shapes and, per case and output tensor, err = max |reference f32 - f64 restatement| /
max |f64 restatement| (tests/ref_decoder.py)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import ref_decoder as RD  # noqa: E402  (the case tables, the generators and the f64 restatement)
from make_heatmap_golden import AttrDict, load_reference  # noqa: E402


def to_torch(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def build_modules(th, tu, c):
    dec = tu.TransformerDecoderLayer(RD.D, RD.NHEAD, c["F"], 0.1, "relu", self_posembed=tu.PositionEmbeddingLearned(2, RD.D),
                                     cross_posembed=tu.PositionEmbeddingLearned(2, RD.D))
    heads = th.SeparateHead_Transfusion(RD.D, 64, 1, RD.sep_head_dict(c["heads"]), use_bias=c["bias"])
    dec.load_state_dict(to_torch(RD.decoder_weights(c["seed"], c["F"])), strict=True)
    heads.load_state_dict(to_torch(RD.head_weights(c["seed"], c["heads"], c["bias"])), strict=True)
    return dec.eval(), heads.eval()


def run_e2e(th, tu, dtype):
    """the reference's predict + get_bboxes unbound on a stand-in self with the real decoder and prediction heads"""
    c = RD.E2E
    logits, feat, enc_w, enc_b = (torch.from_numpy(a).to(dtype) for a in RD.e2e_inputs())
    dec, heads = build_modules(th, tu, c)
    enc = torch.nn.Conv1d(c["C"], RD.D, 1)
    with torch.no_grad():
        enc.weight.copy_(enc_w)
        enc.bias.copy_(enc_b)
    s = types.SimpleNamespace()
    s.shared_conv = lambda t: t
    s.heatmap_head = lambda t: logits
    enc = enc.to(dtype)
    s.class_encoding = lambda t: enc(t.to(dtype))           # predict hands it one_hot.float()
    s.decoder, s.prediction_head = dec.to(dtype), heads.to(dtype)
    s.bev_pos = th.TransFusionHead.create_2D_grid(None, c["W"], c["H"]).to(dtype)
    s.nms_kernel_size, s.num_classes, s.num_proposals = 3, c["C"], c["K"]
    s.dataset_name, s.class_names = "nuScenes", None
    s.model_cfg = AttrDict(POST_PROCESSING=AttrDict(RD.E2E_POST))
    s.feature_map_stride, s.voxel_size, s.point_cloud_range = RD.E2E_STRIDE, list(RD.E2E_VOXEL), list(RD.E2E_PCR)
    s.training, s.pseudo_nms_thresh, s.relabel_classes = False, None, False
    s.decode_bbox = lambda *a, **k: th.TransFusionHead.decode_bbox(s, *a, **k)
    with torch.no_grad():
        res = th.TransFusionHead.predict(s, feat, {})
        kept = th.TransFusionHead.get_bboxes(s, {k: v.clone() for k, v in res.items() if k != "dense_heatmap"})
        s.model_cfg = AttrDict(POST_PROCESSING=AttrDict(SCORE_THRESH=-1.0, POST_CENTER_RANGE=[-1e9] * 3 + [1e9] * 3))
        every = th.TransFusionHead.get_bboxes(s, {k: v.clone() for k, v in res.items() if k != "dense_heatmap"})
    return s.query_labels.numpy(), kept, every


def e2e_case(th, tu, save):
    c = RD.E2E
    labels32, kept32, all32 = run_e2e(th, tu, torch.float32)
    labels64, kept64, all64 = run_e2e(th, tu, torch.float64)
    assert np.array_equal(labels32, labels64), "the f32 and the f64 run select different proposals"
    boxes32 = np.stack([d["pred_boxes"].numpy() for d in all32])
    boxes64 = np.stack([d["pred_boxes"].numpy() for d in all64])
    scores32 = np.stack([d["pred_scores"].numpy() for d in all32])
    scores64 = np.stack([d["pred_scores"].numpy() for d in all64])
    assert boxes32.shape == (c["B"], c["K"], 9)
    err_c = float(np.abs(boxes32[..., :2] - boxes64[..., :2]).max() / np.abs(boxes64[..., :2]).max())
    err_s = float(np.abs(scores32 - scores64).max() / np.abs(scores64).max())
    # the keep decisions are no matter of rounding: no score within 8 x err of the threshold, no centre within that of a limit
    lim = np.asarray(RD.E2E_POST["POST_CENTER_RANGE"], np.float64)
    assert np.abs(scores64 - RD.E2E_POST["SCORE_THRESH"]).min() > 8 * err_s * np.abs(scores64).max()
    for j in range(2):
        gap = np.minimum(np.abs(boxes64[..., j] - lim[j]), np.abs(boxes64[..., j] - lim[3 + j])).min()
        assert gap > 8 * err_c * np.abs(boxes64[..., :2]).max(), gap
    assert (boxes64[..., 2] > lim[2] + 1).all() and (boxes64[..., 2] < lim[5] - 1).all()
    mask = np.zeros((c["B"], c["K"]), bool)
    for b in range(c["B"]):
        rows, j = kept32[b]["pred_boxes"].numpy(), 0
        for k in range(c["K"]):
            if j < rows.shape[0] and np.array_equal(boxes32[b, k], rows[j]):
                mask[b, k], j = True, j + 1
        assert j == rows.shape[0]
        assert np.array_equal(kept64[b]["pred_boxes"].numpy(), boxes64[b][mask[b]]), "the f64 run keeps other queries"
    assert 5 < mask.sum() < mask.size - 5 and (boxes64[..., 0] < lim[0]).any(), "both tests must take part in the decisions"
    save.update(e2e_query_labels=labels32, e2e_keep=mask, e2e_boxes=boxes32, e2e_scores=scores32, e2e_boxes64=boxes64,
                e2e_scores64=scores64, e2e_labels=np.stack([d["pred_labels"].numpy() for d in all32]).astype(np.int32),
                e2e_err_center=np.array([err_c]), e2e_err_score=np.array([err_s]),
                e2e_crc=np.array([RD.crc(a) for a in RD.e2e_inputs()], np.int64))
    print("e2e: kept", mask.sum(1).tolist(), "of", c["K"], "err centre", err_c, "score", err_s)


def main():
    torch.set_num_threads(8)
    th, _, _, tu = load_reference()
    torch.Tensor.cuda = lambda self, *a, **k: self          # decode_bbox's range tensor stays on the CPU (this script only)
    save = {}
    e2e_case(th, tu, save)
    for name, c in RD.LAYER_CASES.items():
        dec, heads = build_modules(th, tu, c)
        query, key, query_pos, bev_pos = RD.layer_inputs(name)
        with torch.no_grad():
            qp = torch.from_numpy(query_pos)
            x = dec(torch.from_numpy(query), torch.from_numpy(key), qp, torch.from_numpy(bev_pos).repeat(c["B"], 1, 1))
            res = heads(x)
            res["center"] = res["center"] + qp.permute(0, 2, 1)
        got = {k: v.numpy() for k, v in res.items()}
        got["query_feat"] = x.contiguous().numpy()
        want = RD.layer_case64(name)
        for k, v in got.items():
            save[f"{name}_{k}"] = v.astype(np.float32)
            save[f"{name}_err_{k}"] = np.array([RD.rel_err(v, want[k])])
        save[name + "_crc"] = np.array([RD.crc(a) for a in (query, key, query_pos, bev_pos)], np.int64)
        print(name, {k: float(save[f"{name}_err_{k}"][0]) for k in got})
        if name == "mid":
            for tag, m in (("decoder", dec), ("heads", heads)):
                sd = m.state_dict()
                save[tag + "_keys"] = np.array(list(sd))
                save[tag + "_shapes"] = np.array(["x".join(str(s) for s in v.shape) for v in sd.values()])
    eye = torch.eye(RD.D)
    for name, c in RD.ATT_CASES.items():
        mha = torch.nn.MultiheadAttention(RD.D, RD.NHEAD, dropout=0.1).eval()
        with torch.no_grad():
            mha.in_proj_weight.copy_(torch.cat([eye, eye, eye]))
            mha.in_proj_bias.zero_()
            mha.out_proj.weight.copy_(eye)
            mha.out_proj.bias.zero_()
            q, k, v = (torch.from_numpy(a) for a in RD.attention_inputs(name))
            out = mha(q.permute(1, 0, 2), k.permute(1, 0, 2), value=v.permute(1, 0, 2))[0].permute(1, 0, 2).contiguous().numpy()
        save[name + "_out"] = out
        save[name + "_err_out"] = np.array([RD.rel_err(out, RD.attention_case64(name))])
        save[name + "_crc"] = np.array([RD.crc(a) for a in RD.attention_inputs(name)], np.int64)
        print(name, float(save[name + "_err_out"][0]))
    np.savez_compressed(RD.GOLDEN, **save)
    print(len(save), "arrays,", os.path.getsize(RD.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
