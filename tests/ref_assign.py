"""Reference helpers for the Hungarian assignment and the per-query targets (csrc/tfassign.hip, csrc/lsap.h): a Python
restatement of scipy's shortest-augmenting-path solver with the matrices the CPU and GPU tests share, and (second half) the case
table of the fixture, f64 evaluations of decode, cost and encode, and the first-order bounds the tests hold the kernels to.

The restatement is scipy >= 1.4's rectangular_lsap, statement for statement: the transpose of a tall matrix, `remaining`
starting as nc-1 .. 0 and shrinking by a swap with its last entry, the reduced cost ((minVal + c) - u[i]) - v[j] in f64, and the
scan's tie rule.  An optimal solver that differs in any of these returns another of the tied assignments."""
import numpy as np


def lsap(cost):
    """linear_sum_assignment(cost) -> (rows, cols), rows ascending."""
    cost = np.asarray(cost, dtype=np.float64)
    nr, nc = cost.shape
    if nr == 0 or nc == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    transpose = nc < nr
    if transpose:
        cost = cost.T.copy()
        nr, nc = nc, nr
    inf = np.inf
    u, v = [0.0] * nr, [0.0] * nc
    col4row, row4col, path = [-1] * nr, [-1] * nc, [-1] * nc
    c = cost.tolist()
    for cur in range(nr):
        min_val = 0.0
        remaining = [nc - 1 - it for it in range(nc)]
        nrem = nc
        SR, SC = [False] * nr, [False] * nc
        spc = [inf] * nc
        sink, i = -1, cur
        while sink == -1:
            SR[i] = True
            lowest, index = inf, -1
            ci, ui = c[i], u[i]
            for it in range(nrem):
                j = remaining[it]
                r = ((min_val + ci[j]) - ui) - v[j]
                if r < spc[j]:
                    path[j] = i
                    spc[j] = r
                if spc[j] < lowest or (spc[j] == lowest and row4col[j] == -1):
                    lowest = spc[j]
                    index = it
            min_val = lowest
            assert index >= 0 and min_val < inf, "no finite assignment"
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            SC[j] = True
            nrem -= 1
            remaining[index] = remaining[nrem]
        u[cur] += min_val
        for i in range(nr):
            if SR[i] and i != cur:
                u[i] += min_val - spc[col4row[i]]
        for j in range(nc):
            if SC[j]:
                v[j] -= min_val - spc[j]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    col4row = np.asarray(col4row, dtype=np.int64)
    if transpose:
        order = np.argsort(col4row)
        return col4row[order], order.astype(np.int64)
    return np.arange(nr, dtype=np.int64), col4row


# ---- the matrices -----------------------------------------------------------------------------------------------------------
# Forms: "normal" (distinct with probability 1), "01" and "012" (heavy ties: most assignments are optimal, so only scipy's scan
# order and tie rule pick one), "int" (integers 0..3), "dup" (normal with duplicated columns: tied columns, distinct rows).

FORMS = ("normal", "01", "012", "int", "dup")


def matrix(rng, nr, nc, form):
    if form == "normal":
        m = rng.standard_normal((nr, nc))
    elif form == "01":
        m = rng.integers(0, 2, (nr, nc))
    elif form == "012":
        m = rng.integers(0, 3, (nr, nc))
    elif form == "int":
        m = rng.integers(0, 4, (nr, nc))
    elif form == "dup":
        m = rng.standard_normal((nr, nc))
        for _ in range(max(1, nc // 5)):
            a, b = rng.integers(0, nc, 2)
            m[:, a] = m[:, b]
    else:
        raise ValueError(form)
    return np.ascontiguousarray(m, dtype=np.float32)


def random_rectangular(seed, count, form, lo=1, hi=40):
    """`count` matrices of `form` with both sides drawn from lo..hi: both orientations and squares occur."""
    rng = np.random.default_rng(seed)
    return [matrix(rng, int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1)), form) for _ in range(count)]


def fixed_cases():
    """The named matrices of the solver tests."""
    rng = np.random.default_rng(77)
    dup = matrix(rng, 200, 37, "normal")
    for a, b in zip(range(30, 37), (0, 3, 5, 9, 11, 20, 20)):      # 7 duplicated columns, one of them duplicated twice
        dup[:, a] = dup[:, b]
    return {
        "200x37 dup7": dup,
        "200x60 int": matrix(rng, 200, 60, "int"),
        "1x1": matrix(rng, 1, 1, "normal"),
        "1x9": matrix(rng, 1, 9, "normal"),
        "9x1": matrix(rng, 9, 1, "normal"),
        "1x9 ties": matrix(rng, 1, 9, "01"),
        "9x1 ties": matrix(rng, 9, 1, "01"),
    }


# ---- cost, targets: cases, f64 evaluations and first-order bounds ---------------------------------------------------------------
# The fixture tests/golden/assign_golden.npz is the reference's own get_targets run on the CPU (make_assign_golden.py).  What
# follows evaluates the same mathematics in f64 with numpy, written from the formulas, and bounds the distance of an f32
# evaluation from it the way ref_heatmap.py does: u = 2^-24 per f32 rounding, and stated factors for the library functions.

import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assign_golden.npz")
U = 2.0 ** -24
F_FUNC = 4 * U        # exp, log, sin, cos, atan2 in f32: within 2 ulp = 4u relative (glibc / sleef / ocml all claim <= 2 ulp)
F_SIGMOID = 6 * U     # exp (4u), the addition and the division (u each)

STRIDE, VOXEL, RANGE = 8, (0.075, 0.075, 0.2), (-54.0, -54.0, -5.0, 54.0, 54.0, 3.0)
ASSIGNER = dict(cls_cost=dict(weight=0.15, alpha=0.25, gamma=2.0, eps=1e-12), reg_cost=dict(weight=0.25), iou_cost=dict(weight=0.25))
HEAD_DIMS = (("heatmap", None), ("center", 2), ("height", 1), ("dim", 3), ("rot", 2), ("vel", 2))

# valid: valid rows per scene; the rows are spread over Mcap with padding rows (all zero) between them
CASES = {
    "main": dict(seed=3, K=200, C=10, Mcap=48, code=10, valid=(0, 5, 37), unknown_labels=(4, 9), bad_rows=1),
    "tall": dict(seed=8, K=64, C=3, Mcap=72, code=8, valid=(70,), unknown_labels=(), bad_rows=0),
}


def head_order(name):
    return ["center", "height", "dim", "rot"] + (["vel"] if CASES[name]["code"] == 10 else [])


def loss_weights(name):
    """LOSS_CONFIG.LOSS_WEIGHTS of a case: the unknown weights only where the case has unknown labels"""
    code = CASES[name]["code"]
    w = dict(code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2][:code])
    if CASES[name]["unknown_labels"]:
        w.update(unknown_cls_weight=0.4, unknown_code_weights=[1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 0.25, 0.25, 0.0, 0.0][:code])
    return w


def case_inputs(name, seed=None):
    """-> preds {head: (B, n, K) f32}, gt_boxes (B, Mcap, code) f32.  Most valid boxes get a query near them (as the heatmap
    proposals do), the other queries are scattered; `bad_rows` rows per scene carry dx <= 0 with a real label."""
    cfg = CASES[name]
    rng = np.random.default_rng(cfg["seed"] if seed is None else seed)
    K, C, Mcap, code, B = cfg["K"], cfg["C"], cfg["Mcap"], cfg["code"], len(cfg["valid"])
    gt = np.zeros((B, Mcap, code), np.float64)
    preds = {h: np.zeros((B, C if n is None else n, K)) for h, n in HEAD_DIMS if h != "vel" or code == 10}
    cell = [STRIDE * VOXEL[0], STRIDE * VOXEL[1]]
    for b, nv in enumerate(cfg["valid"]):
        rows = np.sort(rng.choice(Mcap, nv, replace=False))
        box = np.zeros((nv, code))
        box[:, 0:2] = rng.uniform(-50, 50, (nv, 2))
        box[:, 2] = rng.uniform(-2.5, 0.5, nv)
        box[:, 3:6] = np.exp(rng.uniform(np.log(0.6), np.log(6.0), (nv, 3)))
        box[:, 6] = rng.uniform(-np.pi, np.pi, nv)
        if code == 10:
            box[:, 7:9] = rng.normal(0, 2, (nv, 2))
        box[:, -1] = rng.integers(1, C + 1, nv)
        gt[b, rows] = box
        free = np.setdiff1d(np.arange(Mcap), rows)
        for r in free[:cfg["bad_rows"]]:
            gt[b, r] = box[0] if nv else 0
            gt[b, r, 3], gt[b, r, -1] = -1.0, 1 + r % C
        xy = rng.uniform(-52, 52, (K, 2))
        z, dims, yaw = rng.uniform(-3, 1, K), rng.uniform(np.log(0.5), np.log(7.0), (K, 3)), rng.uniform(-np.pi, np.pi, K)
        logit = rng.normal(-2.5, 1.2, (C, K))
        near = rng.permutation(K)[:min(nv, K)]
        src = rng.permutation(nv)[:near.size]
        xy[near] = box[src, 0:2] + rng.normal(0, 0.5, (near.size, 2))
        z[near] = box[src, 2] + rng.normal(0, 0.2, near.size)
        dims[near] = np.log(box[src, 3:6]) + rng.normal(0, 0.15, (near.size, 3))
        yaw[near] = box[src, 6] + rng.normal(0, 0.2, near.size)
        logit[box[src, -1].astype(int) - 1, near] += rng.uniform(1.0, 4.0, near.size)
        preds["heatmap"][b] = logit
        preds["center"][b] = ((xy - np.array(RANGE[0:2])) / np.array(cell)).T
        preds["height"][b, 0] = z
        preds["dim"][b] = dims.T
        amp = rng.uniform(0.7, 1.3, K)
        preds["rot"][b, 0], preds["rot"][b, 1] = amp * np.sin(yaw), amp * np.cos(yaw)
        if code == 10:
            preds["vel"][b] = rng.normal(0, 2, (2, K))
    return {h: v.astype(np.float32) for h, v in preds.items()}, gt.astype(np.float32)


def valid_rows(gt_scene, C):
    g = gt_scene.astype(np.float64)
    lab = g[:, -1]
    ok = (g[:, 3] > 0) & (g[:, 4] > 0) & (lab >= 1) & (lab < C + 1) & np.isfinite(g[:, [0, 1, 3, 4]]).all(1)
    return np.flatnonzero(ok)


def decode_f64(preds, b):
    """(K, 7 or 9) f64 decoded boxes of scene b and the per-element bound of an f32 decode: the centres take two products and a
    sum (3u of the largest intermediate), exp and atan2 their stated factor, the copies nothing."""
    p = {h: v[b].astype(np.float64) for h, v in preds.items()}
    K = p["center"].shape[1]
    box = np.zeros((K, 9 if "vel" in p else 7))
    bound = np.zeros_like(box)
    for a in range(2):
        box[:, a] = p["center"][a] * STRIDE * VOXEL[a] + RANGE[a]
        bound[:, a] = 3 * U * (np.abs(p["center"][a] * STRIDE * VOXEL[a]) + np.abs(box[:, a]))
    box[:, 2] = p["height"][0]
    box[:, 3:6] = np.exp(p["dim"].T)
    box[:, 6] = np.arctan2(p["rot"][0], p["rot"][1])
    bound[:, 3:7] = F_FUNC * np.abs(box[:, 3:7])
    if "vel" in p:
        box[:, 7:9] = p["vel"].T
    return box, bound


def cls_reg_f64(logits_scene, boxes, gts, labels0, cfg=ASSIGNER):
    """cls + reg of hungarian_assigner.py:61-85 in f64 for boxes (K, 7+), gts (M, 7+), labels0 (M) 0-based -> (K, M) value and
    the bound of an f32 evaluation of the same sequence on the same boxes (module comment of the test: every term below is one
    rounding, u relative, or a stated function factor, propagated to first order)."""
    c = cfg["cls_cost"]
    w, alpha, eps = c["weight"], c["alpha"], c["eps"]
    x = logits_scene.astype(np.float64).T[:, labels0]                   # (K, M)
    p = 1 / (1 + np.exp(-x))
    q = 1 - p
    dp = F_SIGMOID * p
    dq = dp + U * q
    Lp, Lq = -np.log(p + eps), -np.log(q + eps)
    dLp = (dp + U * (p + eps)) / (p + eps) + F_FUNC * np.abs(Lp)
    dLq = (dq + U * (q + eps)) / (q + eps) + F_FUNC * np.abs(Lq)
    pos, neg = Lp * alpha * q ** 2, Lq * (1 - alpha) * p ** 2
    dpos = dLp * alpha * q ** 2 + Lp * alpha * 2 * q * dq + 4 * U * np.abs(pos)      # alpha's rounding and three products
    dneg = dLq * (1 - alpha) * p ** 2 + Lq * (1 - alpha) * 2 * p * dp + 4 * U * np.abs(neg)
    cls = (pos - neg) * w
    dcls = (dpos + dneg + U * np.abs(pos - neg)) * w + 2 * U * np.abs(cls)
    r0, r1 = np.array(RANGE[0:2]), np.array(RANGE[3:5]) - np.array(RANGE[0:2])
    nq, ng = (boxes[:, None, 0:2] - r0) / r1, (gts[None, :, 0:2].astype(np.float64) - r0) / r1
    d = np.abs(nq - ng)
    dd = 3 * U * (np.abs(nq) + np.abs(ng)) + U * d                       # per side: subtraction, range, division; then the difference
    s = d.sum(-1)
    wr = cfg["reg_cost"]["weight"]
    reg = s * wr
    dreg = (dd.sum(-1) + U * s) * wr + 2 * U * np.abs(reg)
    return cls + reg, dcls + dreg + U * np.abs(cls + reg)


def height_volume_f64(boxes, gts):
    """the parts of overlaps() around the BEV term, f64: height overlap (z is the bottom), the two volumes"""
    b, g = boxes.astype(np.float64), gts.astype(np.float64)
    top = np.minimum((b[:, 2] + b[:, 5])[:, None], (g[:, 2] + g[:, 5])[None])
    bot = np.maximum(b[:, 2][:, None], g[:, 2][None])
    return np.clip(top - bot, 0, None), (b[:, 3] * b[:, 4] * b[:, 5])[:, None], (g[:, 3] * g[:, 4] * g[:, 5])[None]


def iou_bound(boxes, gts, bev, box_bound):
    """First-order bound on |iou3d(f32 route A) - iou3d(f32 route B)| where the routes differ in how the QUERY box was decoded
    (box_bound: per-element distance bound of either decode from the f64 one, so the two decodes lie 2 * box_bound apart) and in
    their f32 sin / cos / atan2 inside the overlap.  A rectangle whose boundary moves by at most `disp` changes an intersection
    area by at most (its perimeter) * disp.  disp: half the change of the sides, the centre's, the half diagonal times the yaw's
    change, and the rounding of the corner and crossing-point arithmetic: 16 operations on coordinates up to 64 m.  The fan
    sum adds up to 24 products of coordinates relative to the first vertex, each within the two diagonals' square."""
    b, g = boxes.astype(np.float64), gts.astype(np.float64)
    e = 2 * box_bound
    diag_q, diag_g = np.hypot(b[:, 3], b[:, 4]), np.hypot(g[:, 3], g[:, 4])
    disp = (e[:, 3] + e[:, 4]) / 2 + e[:, 0] + e[:, 1] + diag_q / 2 * (e[:, 6] + 2 * F_FUNC * np.pi) + 16 * U * 64
    disp_g = diag_g / 2 * 2 * F_FUNC * np.pi + 16 * U * 64
    per_q, per_g = 2 * (b[:, 3] + b[:, 4]), 2 * (g[:, 3] + g[:, 4])
    dA = per_g[None] * disp[:, None] + per_q[:, None] * disp_g[None] + 24 * U * (diag_q[:, None] + diag_g[None]) ** 2 + 2 * U * bev
    h, vq, vg = height_volume_f64(b, g)
    dh = (e[:, 2] * 2 + e[:, 5])[:, None] + 3 * U * (np.abs(b[:, 2]) + b[:, 5])[:, None] + 3 * U * (np.abs(g[:, 2]) + g[:, 5])[None]
    o3 = bev * h
    do3 = dA * h + bev * dh + U * o3
    dvq = (vq[:, 0] * (e[:, 3] / b[:, 3] + e[:, 4] / b[:, 4] + e[:, 5] / b[:, 5]))[:, None] + 2 * U * vq
    den = np.maximum(vq + vg - o3, 1e-8)
    dden = dvq + 2 * U * vg + do3 + 2 * U * (vq + vg)
    iou = o3 / den
    return do3 / den + iou * dden / den + U * iou


def encode_f64(rows):
    """encode_bbox (transfusion_head.py:604-614) of gt boxes (n, code - 1: no label column) in f64 -> targets (n, code), bound (n, code) of an f32
    evaluation: the two cell coordinates take a subtraction, the divisor's rounding and a division; log, sin, cos their factor."""
    g = rows.astype(np.float64)
    code = g.shape[1] + 1
    t, bound = np.zeros((g.shape[0], code)), np.zeros((g.shape[0], code))
    for a in range(2):
        t[:, a] = (g[:, a] - RANGE[a]) / (STRIDE * VOXEL[a])
        bound[:, a] = 3 * U * np.abs(t[:, a])
    t[:, 2] = g[:, 2]
    t[:, 3:6] = np.log(g[:, 3:6])
    t[:, 6], t[:, 7] = np.sin(g[:, 6]), np.cos(g[:, 6])
    bound[:, 3:8] = F_FUNC * np.abs(t[:, 3:8])
    if code == 10:
        t[:, 8:10] = g[:, 7:9]
    return t, bound


_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


# ---- the two query losses: f64 evaluation with gradients and first-order bounds of an f32 evaluation ------------------------------

ALPHA, GAMMA = 0.25, 2.0


def fixture_targets(name):
    g = golden()
    return {k: g[f"{name}_{k}"] for k in ("labels", "label_weights", "bbox_targets", "bbox_weights", "unknown_mask", "num_pos")}


def loss_f64(name, preds, targets, out_ulp=0.0):
    """preds {head: (B, n, K)} (any float dtype, widened exactly), targets as the fixture holds them -> dict with loss_cls, loss_bbox
    (f64), grad_<head> (B, n, K) of loss_cls + loss_bbox, and the bounds bound_loss_cls, bound_loss_bbox, bound_grad_<head> of an
    f32 evaluation (gamma = 2).  Per element, to first order: p carries F_SIGMOID relative, q = 1 - p that plus a rounding; a product
    or sum adds u; exp and log1p carry F_FUNC; bce = (max(x, 0) - x t) + log1p(exp(-|x|)) is bounded term by term (absolutely: it
    does not cancel); the two terms of the derivative are bounded separately because they can cancel.  The f64 partial sums add
    nothing visible; the final rounding of a loss adds u.  out_ulp: the relative half-spacing of the dtype the gradients are stored
    in (0 for f32, whose rounding is already counted; 2^-11 for f16, 2^-8 for bf16)."""
    w_cfg = loss_weights(name)
    x = preds["heatmap"].astype(np.float64).transpose(0, 2, 1)                    # (B, K, C)
    B, K, C = x.shape
    unk = targets["unknown_mask"].astype(bool)
    den = max(int(targets["num_pos"]), 1)
    hit = targets["labels"][..., None] == np.arange(C)
    f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)     # the weights are f32 tensors in the reference, whatever the run
    w = targets["label_weights"].astype(np.float64) * np.where(unk, f32(w_cfg.get("unknown_cls_weight", 1.0)), 1.0)
    w = w[..., None]
    p = 1 / (1 + np.exp(-x))
    q = 1 - p
    rp = F_SIGMOID
    dq = rp * p + U * q
    pt, rpt = np.where(hit, q, p), np.where(hit, dq / q, rp)
    aw = np.where(hit, ALPHA, 1 - ALPHA)
    e = np.exp(-np.abs(x))
    lin, L = np.maximum(x, 0) - np.where(hit, x, 0), np.log1p(e)
    bce = lin + L
    dbce = U * np.abs(lin) + F_FUNC * e / (1 + e) + F_FUNC * L + U * bce
    ptg = pt * pt
    elem = aw * ptg * bce * w
    d_elem = elem * (2 * rpt + 5 * U) + aw * ptg * w * dbce
    out = {"loss_cls": elem.sum() / den}
    out["bound_loss_cls"] = d_elem.sum() / den + 2 * U * abs(out["loss_cls"])
    dpt = np.where(hit, -1.0, 1.0) * p * q
    r_dpt = rp + dq / q + U
    T1 = 2 * pt * dpt * bce
    dT1 = np.abs(T1) * (rpt + r_dpt + 3 * U) + np.abs(2 * pt * dpt) * dbce
    pmt = np.where(hit, -q, p)
    T2 = ptg * pmt
    dT2 = np.abs(T2) * (2 * rpt + 2 * U) + ptg * np.where(hit, dq, rp * p)
    dl = aw * (T1 + T2)
    d_dl = aw * (dT1 + dT2 + U * np.abs(T1 + T2)) + 2 * U * np.abs(dl)
    g = dl * w / den
    out["grad_heatmap"] = g.transpose(0, 2, 1)
    out["bound_grad_heatmap"] = (d_dl * w / den + (4 * U + out_ulp) * np.abs(g)).transpose(0, 2, 1)
    order = head_order(name)
    pred = np.concatenate([preds[h].astype(np.float64) for h in order], 1).transpose(0, 2, 1)     # (B, K, code)
    rw = targets["bbox_weights"].astype(np.float64) * f32(w_cfg["code_weights"])
    if "unknown_code_weights" in w_cfg:
        rw = np.where(unk[..., None], rw * f32(w_cfg["unknown_code_weights"]), rw)
    d = pred - targets["bbox_targets"].astype(np.float64)
    eb = np.abs(d) * rw
    out["loss_bbox"] = eb.sum() / den
    out["bound_loss_bbox"] = (5 * U * eb).sum() / den + 2 * U * out["loss_bbox"]      # the difference, the two weights' products, the product
    gb = (np.sign(d) * rw / den).transpose(0, 2, 1)
    at = 0
    for h in order:
        n = preds[h].shape[1]
        out["grad_" + h] = gb[:, at:at + n]
        out["bound_grad_" + h] = (5 * U + out_ulp) * np.abs(gb[:, at:at + n])
        at += n
    return out
