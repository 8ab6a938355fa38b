"""CPU restatement of TransFusionHead's inference side around the decoder (transfusion_head.py:201-324 proposals and query
initialisation, :616-728 get_bboxes + decode_bbox(filter=True)), the case table and the seeded input generators.  It is the
yardstick of tests/test_proposals_ref.py (held to the reference's own output in tests/golden/proposals_golden.npz) and, where
the reference's order is not defined (ties, zero fill), of tests/test_gpu_proposals.py.

ORDER: masked value descending, then flat index c*H*W + h*W + w ascending = torch.sort(stable=True, descending=True).  The
reference's argsort(descending=True) is not stable; on distinct values both give the same order.  Masked-out cells take part
with value 0, so with P < K positive cells the places behind them go to the lowest flat indices that are no positive cell.

FUSED SIGMOID BOUND (the `sigmoid` case: logits a permutation of linspace(-6, 2, 10*32*32), neighbouring f64 sigmoids >= 780
f32 ulps apart, so no rounding reorders them): the device's 1.0f / (1.0f + expf(-x)) is held to the f64 sigmoid of the f32 logit
within SIGMOID_REF_ULP (the error of the reference's own CPU f32 sigmoid against f64 on these inputs, recorded by the generator
in the fixture as `sigmoid_ref_ulp`; 1.8 ulp when the fixture was made, read back from the fixture by the test) + SIGMOID_EXTRA_ULP = 2 ulps for expf and
the division: 3.79 ulp.  Observed on one MI355X: 1.17 ulp.  Elsewhere (the `zerofill` case's 37 logits) the scores are
held to SIGMOID_FIRST_ORDER_ULP = 4: expf carries 1 ulp in the HIP math API's table, at most 2u relative (u = 2^-24), times
e / (1 + e) <= 1, + u for the sum + u for the division = 4u relative, and u relative is at most one ulp (ref_heatmap.py, A = 4).

DECODE BOUNDS: scores, sizes and yaw against the f64 evaluation of the same span; the allowance is twice the reference's own
f32-against-f64 error on the same inputs, per quantity, recorded in the fixture (`<case>_err_ulp` = score, size, yaw).  The
case generator asserts that no f64 score lies within that allowance of its threshold and that no centre meets a range limit
except the two queries put exactly on the inclusive limits (from exactly representable values), so no keep decision hinges on
a rounding."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

f32 = np.float32
SIGMOID_EXTRA_ULP = 2.0
SIGMOID_FIRST_ORDER_ULP = 4.0
NUSC10 = dict(dataset_name="nuScenes", class_names=None)

# ---- proposals: the case table ------------------------------------------------------------------------------------------
# kind: how the map is generated; from_logits: the fused-sigmoid path; exact: the reference's order is defined (>= K positive
# survivors, no ties among them), so the fixture decides; otherwise the restatement does.
CASES = {
    "small_b1": dict(B=1, C=10, H=24, W=40, K=200, kind="distinct", seed=1, from_logits=False, exact=True, **NUSC10),
    "small_b3": dict(B=3, C=10, H=24, W=40, K=200, kind="distinct", seed=2, from_logits=False, exact=True, **NUSC10),
    "ties": dict(B=2, C=10, H=24, W=40, K=200, kind="ties", seed=3, from_logits=False, exact=False, **NUSC10),
    "zerofill": dict(B=2, C=10, H=24, W=40, K=200, kind="zerofill", seed=4, from_logits=True, exact=False, **NUSC10),
    "borders": dict(B=1, C=10, H=24, W=40, K=200, kind="borders", seed=5, from_logits=False, exact=True, **NUSC10),
    "waymo": dict(B=2, C=3, H=16, W=16, K=50, kind="distinct", seed=6, from_logits=False, exact=True, dataset_name="Waymo", class_names=None),
    "kitti": dict(B=2, C=3, H=16, W=16, K=50, kind="distinct", seed=7, from_logits=False, exact=True, dataset_name="kitti",
                  class_names=["Car", "Pedestrian", "Cyclist"]),
    "refine": dict(B=1, C=10, H=48, W=64, K=200, kind="refine", seed=8, from_logits=False, exact=False, **NUSC10),
    "full_k200": dict(B=1, C=10, H=180, W=180, K=200, kind="distinct", seed=9, from_logits=False, exact=True, **NUSC10),
    "full_k500": dict(B=1, C=10, H=180, W=180, K=500, kind="distinct", seed=9, from_logits=False, exact=True, **NUSC10),
    "sigmoid": dict(B=1, C=10, H=32, W=32, K=200, kind="sigmoid", seed=10, from_logits=True, exact=True, **NUSC10),
}
BORDER_ORDINARY = (0, 0, 5)      # (class, h, w): a peak on the border of an ordinary class: never selected
BORDER_POINT = (8, 0, 7)         # a peak on the border of a point class: selected first
QUERY_FEATURES = 16              # channels of lidar_feat in the query-initialisation case
QUERY_CASE = "small_b3"


def point_classes(cfg):
    if cfg["dataset_name"] == "nuScenes" and cfg["C"] == 10:
        return [8, 9]
    if cfg["dataset_name"] == "Waymo":
        return [1, 2]
    if cfg["dataset_name"] == "kitti":
        return [i for i, n in enumerate(cfg["class_names"]) if n in ("Pedestrian", "Person_Sitting", "Cyclist")]
    return []


def case_map(name):
    """the case's (B, C, H, W) f32 map: probabilities, or logits when the case is from_logits"""
    c = CASES[name]
    B, C, H, W = c["B"], c["C"], c["H"], c["W"]
    n = B * C * H * W
    rng = np.random.default_rng(c["seed"])
    kind = c["kind"]
    if kind in ("distinct", "borders"):
        x = ((rng.permutation(n) + 0.5) / n).astype(f32)             # n < 2^24: all distinct, in (0, 1)
        x = x.reshape(B, C, H, W)
        if kind == "borders":
            x *= f32(0.5)
            x[0][BORDER_ORDINARY] = f32(0.99)
            x[0][BORDER_POINT] = f32(0.98)
        assert np.unique(x).size == n
        return x
    if kind == "ties":
        x = (rng.integers(0, 65, n) / 64.0).astype(f32).reshape(B, C, H, W)
        x[:, 0, 6:11, 28:37] = 1.0                                    # plateaus across the 32-wide and 8-high tile borders
        x[:, 8, 5:10, 30:35] = 1.0
        x[:, 3, 14:18, 0:4] = 0.75
        return x
    if kind == "zerofill":
        x = np.full((B, C, H, W), -200.0, f32)
        for b in range(B):
            cells = rng.choice(C * H * W, 37, replace=False)
            cells[:5] = np.arange(41, 46) + b                         # flat indices below K: the fill has to step over them
            x[b].reshape(-1)[cells] = rng.normal(0, 2, 37).astype(f32)
        return x
    if kind == "refine":
        return (0.5 + rng.random(n) * 1e-4).astype(f32).clip(0.5, 0.5001).reshape(B, C, H, W)
    if kind == "sigmoid":
        return rng.permutation(np.linspace(-6, 2, n)).astype(f32).reshape(B, C, H, W)
    raise KeyError(kind)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def masked_map(x, cfg, from_logits=None):
    """-> the masked values (B, C, H*W) as an f32 torch tensor: predict :201-287 with the CPU's f32 sigmoid"""
    t = torch.from_numpy(np.ascontiguousarray(x))
    heat = t.sigmoid() if (cfg["from_logits"] if from_logits is None else from_logits) else t
    B, C, H, W = heat.shape
    local_max = torch.zeros_like(heat)
    local_max[:, :, 1:-1, 1:-1] = F.max_pool2d(heat, kernel_size=3, stride=1, padding=0)
    for c in point_classes(cfg):
        local_max[:, c] = heat[:, c]
    return (heat * (heat == local_max)).view(B, C, H * W)


def proposals(x, cfg, from_logits=None):
    """the restatement of A -> top_class, top_index (B, K) int64, top_score (B, K) f32, query_heatmap_score (B, C, K) f32"""
    m = masked_map(x, cfg, from_logits)
    B, C, HW = m.shape
    vals, order = torch.sort(m.view(B, -1), dim=-1, descending=True, stable=True)
    order, vals = order[:, :cfg["K"]], vals[:, :cfg["K"]]
    top_class, top_index = order // HW, order % HW
    qhs = m.gather(index=top_index[:, None, :].expand(-1, C, -1), dim=-1)
    return top_class.numpy(), top_index.numpy(), vals.numpy(), qhs.numpy()


def bev_pos_table(H, W):
    """create_2D_grid(x_size=W, y_size=H): x-major rows, (x + 0.5, y + 0.5)"""
    xs, ys = np.meshgrid(np.arange(W, dtype=f32) + f32(0.5), np.arange(H, dtype=f32) + f32(0.5), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel()], axis=1)


def query_inputs(name=QUERY_CASE):
    """lidar_feat (B, F, H, W), the class encoding's weight (F, C, 1) and bias (F): seeded"""
    c = CASES[name]
    rng = np.random.default_rng(100 + c["seed"])
    feat = rng.normal(0, 1, (c["B"], QUERY_FEATURES, c["H"], c["W"])).astype(f32)
    w = rng.normal(0, 0.5, (QUERY_FEATURES, c["C"], 1)).astype(f32)
    bias = rng.normal(0, 0.5, QUERY_FEATURES).astype(f32)
    return feat, w, bias


def init_queries(feat_flat, bev_pos, w, bias, top_class, top_index):
    """the restatement of B on numpy arrays: feat_flat (B, F, HW), bev_pos (HW, 2), w (F, C), bias (F)"""
    B, Fd, _ = feat_flat.shape
    qf = np.take_along_axis(feat_flat, np.broadcast_to(top_index[:, None, :], (B, Fd, top_index.shape[1])), axis=2)
    enc = (w[:, top_class] + bias[:, None, None]).transpose(1, 0, 2)   # (B, F, K)
    return (qf + enc).astype(f32), bev_pos[top_index][..., ::-1].astype(f32)


def ulps(got, want64):
    """|got - want| in units of the f32 spacing at want (f64 reference values)"""
    want64 = np.asarray(want64, np.float64)
    sp = np.spacing(np.abs(want64).astype(f32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - want64) / sp


# ---- decode: the case table -----------------------------------------------------------------------------------------------
DECODE_C = 10
DECODE_STRIDE = 8
DECODE_VOXEL = [0.075, 0.25, 0.2]
DECODE_PCR = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
DECODE_POST = dict(SCORE_THRESH=0.1, POST_CENTER_RANGE=[-50.0, -60.0, -10.0, 50.0, 60.0, 10.0])
DECODE_CASES = {
    "dec_b1": dict(B=1, K=200, vel=True, thresh_unk=None, unknown_labels=(), relabel=None, seed=21),
    "dec_b3_novel": dict(B=3, K=200, vel=False, thresh_unk=None, unknown_labels=(), relabel=None, seed=22),
    "dec_b3_unk": dict(B=3, K=200, vel=True, thresh_unk=0.3, unknown_labels=(2, 5, 10), relabel=None, seed=23),
    "dec_b1_relabel": dict(B=1, K=200, vel=True, thresh_unk=None, unknown_labels=(), relabel=[0, 3, 1, 4, 1, 5, 9, 2, 6, 5, 3], seed=24),
}


def decode_post_cfg(c):
    cfg = dict(DECODE_POST)
    if c["thresh_unk"] is not None:
        cfg["SCORE_THRESH_UNK"] = c["thresh_unk"]
    return cfg


def decode_inputs(name):
    """seeded predictions (B, n, K) f32 and query_labels (B, K) int64.  Queries 0 and 1 of every scene sit exactly on the
    inclusive POST_CENTER_RANGE limits in y and z (y = c * 8 * 0.25 - 54 with c = -3 and 57; z = -10 and 10), with a score far
    above the threshold: they are kept.  Every tenth query has a zero query_heatmap_score column (a zero-filled proposal)."""
    c = DECODE_CASES[name]
    B, K, C = c["B"], c["K"], DECODE_C
    rng = np.random.default_rng(c["seed"])
    p = {
        "heatmap": rng.normal(0, 2, (B, C, K)).astype(f32),
        "query_heatmap_score": rng.uniform(0.05, 1, (B, C, K)).astype(f32),
        "center": rng.uniform(-10, 190, (B, 2, K)).astype(f32),
        "height": rng.uniform(-12, 12, (B, 1, K)).astype(f32),
        "dim": rng.normal(0.5, 0.7, (B, 3, K)).astype(f32),
        "rot": rng.normal(0, 1, (B, 2, K)).astype(f32),
    }
    if c["vel"]:
        p["vel"] = rng.normal(0, 3, (B, 2, K)).astype(f32)
    labels = rng.integers(0, C, (B, K)).astype(np.int64)
    p["query_heatmap_score"][:, :, 9::10] = 0
    for q, (cy, z) in enumerate(((-3.0, -10.0), (57.0, 10.0))):
        p["center"][:, 0, q], p["center"][:, 1, q], p["height"][:, 0, q] = 90.0, cy, z
        p["heatmap"][:, :, q], p["query_heatmap_score"][:, :, q] = 4.0, 0.9
    return p, labels


def decode(p, labels, c, dtype=np.float64):
    """the restatement of C in `dtype` -> per-query boxes (B, K, 7|9), scores, 1-based labels (relabelled), keep mask.
    Centres are formed in f32 whatever the dtype (they are held bit for bit); thresholds and range tests in f32."""
    B, C, K = p["heatmap"].shape
    hm = np.take_along_axis(p["heatmap"], labels[:, None, :], axis=1)[:, 0].astype(dtype)
    qs = np.take_along_axis(p["query_heatmap_score"], labels[:, None, :], axis=1)[:, 0].astype(dtype)
    with np.errstate(over="ignore"):
        v = (1 / (1 + np.exp(-hm))) * qs
    label0 = np.where(v > 0, labels, 0)
    cx = p["center"][:, 0] * f32(DECODE_STRIDE) * f32(DECODE_VOXEL[0]) + f32(DECODE_PCR[0])
    cy = p["center"][:, 1] * f32(DECODE_STRIDE) * f32(DECODE_VOXEL[1]) + f32(DECODE_PCR[1])
    cols = [cx.astype(dtype), cy.astype(dtype), p["height"][:, 0].astype(dtype)]
    cols += [np.exp(p["dim"][:, j].astype(dtype)) for j in range(3)]
    cols += [np.arctan2(p["rot"][:, 0].astype(dtype), p["rot"][:, 1].astype(dtype))]
    if "vel" in p:
        cols += [p["vel"][:, 0].astype(dtype), p["vel"][:, 1].astype(dtype)]
    boxes = np.stack(cols, axis=-1)
    unk = np.isin(label0 + 1, np.asarray(list(c["unknown_labels"]), np.int64)) if c["thresh_unk"] is not None else np.zeros_like(label0, bool)
    thresh = np.where(unk, f32(c["thresh_unk"] if c["thresh_unk"] is not None else 0), f32(DECODE_POST["SCORE_THRESH"])).astype(f32)
    rng_ = np.asarray(DECODE_POST["POST_CENTER_RANGE"], f32)
    xyz = boxes[..., :3].astype(f32)
    keep = (v.astype(f32) > thresh) & (xyz >= rng_[:3]).all(-1) & (xyz <= rng_[3:]).all(-1)
    out_labels = label0 + 1
    if c["relabel"] is not None:
        out_labels = np.asarray(c["relabel"], np.int64)[out_labels]
    return boxes, v, out_labels.astype(np.int32), keep, thresh
