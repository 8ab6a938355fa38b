"""numpy restatement of TransFusionHead's dense heatmap targets and heatmap loss (transfusion_head.py:446-470, :492-498), the
yardstick of tests/test_heatmap_ref.py (held to the reference's own output in tests/golden/heatmap_golden.npz) and of
tests/test_gpu_heatmap.py (beyond the fixture's sizes).

PARAMETERS, f32 as torch runs them on the CPU: true IEEE divisions by f32(voxel) and f32(stride); gaussian_radius with the
reference's operand order, its Python scalars formed in f64 and rounded to f32 where they meet the tensor, b**2 as b*b;
r = max(MIN_RADIUS, trunc(min(r1, r2, r3))), an unknown label's r = trunc(double(r) * UNK_RADIUS_MULT); centres truncate toward 0.
WEIGHTS: float32(exp_f64(-(dx^2 + dy^2) / (2 sigma^2))), sigma = (2r + 1) / 6 in f64; gaussian2D's eps threshold never fires
(the smallest weight of a radius is its corner's, about exp(-9)) and is left out.
LOSS: f64, with the clamp at the F32-ROUNDED constants f32(1e-4), f32(1 - 1e-4) (the f64 constants alone are a 250x miss
against any f32 run on saturated elements).

ERROR BOUNDS of an f32 evaluation against that f64 value, first order, u = 2^-24, one u per f32 rounding; expf and logf carry
1 ulp each in the HIP math API's table of single-precision functions, which is at most 2u relative:
  p  = clamp(1 / (1 + expf(-x)))      expf 2u (times e / (1 + e) <= 1) + the sum u + the division u         -> A = 4 (|dp| <= A u p)
  q  = 1 - p                          |dq| <= u (A p + q) =: u DQ
  positive (t == 1)   T = -log(p) q^2          own roundings: logf 2, q*q 1, product 1                       =  4
  other               T = -log(q) p^2 w, w = (1-t)^4   logf 2, p*p 1, 1-t 1, its square 2+1, the fourth power 6+1, two products 2  = 12
      tol_T = u (K |T| + [pos] (A q^2 + DQ 2 q |log p|)  or  [other] w (A p 2 p |log q| + DQ p^2 / q))
  gradient with respect to the logit inside the clamp (outside it is exactly 0), scaled by grad_out / max(num_pos, 1):
  positive            G = -q^3 + 2 p q^2 log p     q*q 1, p*q2 1, logf 2, product 1 (= 5; the cube has 2), the difference of
                                                    two terms of one sign 1, the scale's division 1 and product 1          =  8
  other               G = w (p^3 - 2 p^2 q log q)   p*p 1, p2*q 1, logf 2, product 1 (= 5; the cube has 2), the difference 1, w 7,
                                                    product 1, the scale 2                                                 = 16
      tol_G = u (K |G| + A p |dG/dp| + DQ |dG/dq|)   with   positive: dG/dp = 2 q^2 (log p + 1), dG/dq = -3 q^2 + 4 p q log p
                                                            other:    dG/dp = w (3 p^2 - 4 p q log q), dG/dq = -2 w p^2 (log q + 1)
K = 16 covers every chain above; A = 4."""
import numpy as np

U = 2.0 ** -24
K = 16
A = 4
CLAMP_LO = float(np.float32(1e-4))
CLAMP_HI = float(np.float32(1 - 1e-4))
f32 = np.float32


# ---- targets ---------------------------------------------------------------------------------------------------------

def radius_f32(length, width, overlap):
    """gaussian_radius(height=length, width=width, overlap) on f32 arrays, before truncation"""
    h, w = np.asarray(length, f32), np.asarray(width, f32)
    o = float(overlap)
    with np.errstate(all="ignore"):
        b1 = h + w
        c1 = w * h * f32(1 - o) / f32(1 + o)
        r1 = (b1 + np.sqrt(b1 * b1 - f32(4) * c1)) / f32(2)
        b2 = f32(2) * (h + w)
        c2 = f32(1 - o) * w * h
        r2 = (b2 + np.sqrt(b2 * b2 - f32(16) * c2)) / f32(2)
        a3 = 4 * o
        b3 = f32(-2 * o) * (h + w)
        c3 = f32(o - 1) * w * h
        r3 = (b3 + np.sqrt(b3 * b3 - f32(4 * a3) * c3)) / f32(2)
        return np.minimum(np.minimum(r1, r2), r3)


def box_params(boxes, num_classes, voxel_size, point_cloud_range, stride, overlap, min_radius, unknown_labels=(), unk_mult=1.0):
    """boxes (..., ncol) f32 with the 1-based label last -> (..., 4) int32 {class, cx, cy, r}; class -1 = skipped"""
    boxes = np.asarray(boxes, f32)
    flat = boxes.reshape(-1, boxes.shape[-1])
    out = np.zeros((flat.shape[0], 4), np.int32)
    out[:, 0] = -1
    vx, vy, st = f32(voxel_size[0]), f32(voxel_size[1]), f32(stride)
    with np.errstate(all="ignore"):
        width = flat[:, 3] / vx / st
        length = flat[:, 4] / vy / st
        fx = (flat[:, 0] - f32(point_cloud_range[0])) / vx / st
        fy = (flat[:, 1] - f32(point_cloud_range[1])) / vy / st
        lab = flat[:, -1]
        ok = (flat[:, 3] > 0) & (flat[:, 4] > 0) & (width > 0) & (length > 0) & np.isfinite(width) & np.isfinite(length) \
            & np.isfinite(flat[:, 0]) & np.isfinite(flat[:, 1]) & (lab >= 1) & (lab < num_classes + 1)
    idx = np.nonzero(ok)[0]
    if idx.size:
        r = radius_f32(length[idx], width[idx], overlap)
        ri = np.maximum(int(min_radius), r.astype(np.int64))
        label = lab[idx].astype(np.int64)
        unk = np.isin(label, np.asarray(list(unknown_labels), np.int64))
        ri = np.where(unk, (ri.astype(np.float64) * float(unk_mult)).astype(np.int64), ri)
        out[idx, 0] = label - 1
        out[idx, 1] = fx[idx].astype(np.int64)     # truncation toward zero
        out[idx, 2] = fy[idx].astype(np.int64)
        out[idx, 3] = ri
    return out.reshape(boxes.shape[:-1] + (4,))


def gaussian_f32(radius):
    """the (2r+1, 2r+1) weights of one radius, f32"""
    r = int(radius)
    sigma = (2 * r + 1) / 6
    y, x = np.ogrid[-float(r):r + 1.0, -float(r):r + 1.0]
    return np.exp(-(x * x + y * y) / (2 * sigma * sigma)).astype(f32)


def draw(params, num_classes, H, W):
    """params (M, 4) of one scene -> (C, H, W) f32: elementwise maximum of the clipped windows"""
    hm = np.zeros((num_classes, H, W), f32)
    cache = {}
    for c, x, y, r in np.asarray(params).reshape(-1, 4).tolist():
        if c < 0:
            continue
        x0, x1, y0, y1 = max(0, x - r), min(W, x + r + 1), max(0, y - r), min(H, y + r + 1)
        if x1 <= x0 or y1 <= y0:
            continue
        g = cache.get(r)
        if g is None:
            g = cache[r] = gaussian_f32(r)
        win = hm[c, y0:y1, x0:x1]
        np.maximum(win, g[y0 - y + r:y1 - y + r, x0 - x + r:x1 - x + r], out=win)
    return hm


def targets(gt_boxes, num_classes, grid_size, voxel_size, point_cloud_range, stride, overlap, min_radius, unknown_labels=(), unk_mult=1.0):
    """gt_boxes (B, M, ncol) -> heatmap (B, C, H, W) f32, num_pos, params (B, M, 4)"""
    gt_boxes = np.asarray(gt_boxes, f32)
    W, H = int(grid_size[0]) // int(stride), int(grid_size[1]) // int(stride)
    params = box_params(gt_boxes, num_classes, voxel_size, point_cloud_range, stride, overlap, min_radius, unknown_labels, unk_mult)
    hm = np.zeros((gt_boxes.shape[0], num_classes, H, W), f32)
    for b in range(gt_boxes.shape[0]):
        hm[b] = draw(params[b], num_classes, H, W)
    return hm, int((hm == 1).sum()), params


# ---- loss ------------------------------------------------------------------------------------------------------------

def loss64(x, t, lo=CLAMP_LO, hi=CLAMP_HI, eps=0.0):
    """per-element loss T and gradient G with respect to the logit (of the plain sum), f64, and the pieces the bounds need.
    eps: GaussianFocalLoss's 1e-12 inside both logarithms.  It matters to an f64 run only (in f32 it is below half the spacing
    of any operand >= 1e-4 and vanishes), so the yardstick of an f32 kernel keeps 0; lo, hi, eps as the reference's f64 run has
    them (1e-4, 1 - 1e-4, 1e-12) reproduce that run."""
    x = np.asarray(x).astype(np.float64)
    t = np.asarray(t).astype(np.float64)
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-x))
    inside = (s >= lo) & (s <= hi)
    p = np.clip(s, lo, hi)
    q = 1.0 - p
    pos = t == 1
    w = (1.0 - t) ** 4
    lp, lq = np.log(p + eps), np.log(q + eps)
    T = np.where(pos, -lp * q * q, -lq * p * p * w)
    dTdp = np.where(pos, -q * q / (p + eps) + 2 * q * lp, w * (p * p / (q + eps) - 2 * p * lq))
    G = np.where(inside, dTdp * p * q, 0.0)     # (eps = 0: -q^3 + 2 p q^2 log p, w (p^3 - 2 p^2 q log q))
    return dict(T=T, G=G, p=p, q=q, w=w, pos=pos, inside=inside, lp=lp, lq=lq)


def tol_T(r, k=K, a=A):
    p, q, w, lp, lq = r["p"], r["q"], r["w"], r["lp"], r["lq"]
    dq = a * p + q
    prop = np.where(r["pos"], a * q * q + dq * 2 * q * np.abs(lp), w * (a * p * 2 * p * np.abs(lq) + dq * p * p / q))
    return U * (k * np.abs(r["T"]) + prop)


def tol_G(r, k=K, a=A):
    p, q, w, lp, lq = r["p"], r["q"], r["w"], r["lp"], r["lq"]
    dq = a * p + q
    dGdp = np.where(r["pos"], 2 * q * q * (lp + 1), w * (3 * p * p - 4 * p * q * lq))
    dGdq = np.where(r["pos"], -3 * q * q + 4 * p * q * lp, -2 * w * p * p * (lq + 1))
    return np.where(r["inside"], U * (k * np.abs(r["G"]) + a * p * np.abs(dGdp) + dq * np.abs(dGdq)), 0.0)


def loss_and_bounds(x, t, num_pos, k=K, a=A):
    """loss = sum T / max(num_pos, 1) in f64 with its bound (sum tol_T / n plus two roundings of the result), and the gradient of
    that loss with its elementwise bound"""
    r = loss64(x, t)
    n = max(int(num_pos), 1)
    loss = r["T"].sum() / n
    return dict(loss=loss, loss_tol=tol_T(r, k, a).sum() / n + 2 * U * abs(loss), grad=r["G"] / n, grad_tol=tol_G(r, k, a) / n,
                inside=r["inside"])


def make_logits(rng, shape, lo=-12.0, hi=12.0):
    """f32 logits over [lo, hi], none within 1e-3 of the clamp thresholds |x| = log(1/1e-4 - 1) (the gradient jumps to 0 there
    and an f32 sigmoid may fall on the other side): those are moved 2e-3 further out, none is dropped"""
    x = rng.uniform(lo, hi, shape).astype(f32)
    thr = np.log(1 / 1e-4 - 1)
    near = np.abs(np.abs(x) - thr) < 1e-3
    x[near] = (np.sign(x[near]) * (thr + 2e-3)).astype(f32)
    return x


def make_targets(rng, shape, ones=0.02, between=0.2):
    """f32 targets: exact ones, zeros and values in between"""
    t = np.zeros(shape, f32)
    sel = rng.uniform(0, 1, shape)
    mid = sel < between
    t[mid] = rng.uniform(0, 1, int(mid.sum())).astype(f32)
    t[sel > 1 - ones] = 1.0
    return t


# ---- the fixture's cases (tests/golden/make_heatmap_golden.py runs the reference on them) ---------------------------------

VOXEL_SIZE = (0.075, 0.075, 0.2)
STRIDE = 8
OVERLAP = 0.1
MIN_RADIUS = 2
LOSS_SHAPE = (2, 3, 20, 24)


def _cfg(num_classes, grid_xy=(1440, 1440), unknown_labels=(), unk_mult=1.0):
    half = [g * VOXEL_SIZE[0] / 2 for g in grid_xy]
    return dict(num_classes=num_classes, grid_size=[grid_xy[0], grid_xy[1], 40], unknown_labels=tuple(unknown_labels), unk_mult=unk_mult,
                point_cloud_range=[-half[0], -half[1], -5.0, half[0], half[1], 3.0])


CASES = {
    "a": _cfg(10, (1408, 1600)),                         # non-square: H = 200, W = 176; padded rows between valid ones
    "b": _cfg(3),                                        # centres on and beyond every edge
    "c1": _cfg(10, unknown_labels=(3, 7, 9), unk_mult=1.5),
    "c2": _cfg(10, unknown_labels=(1, 2), unk_mult=2.0),
    "d": _cfg(2),                                        # 700 boxes of one class, overlapping: more than one LDS chunk
    "e": _cfg(1),
    "f0": _cfg(10),                                      # a scene with no box
    "f1": _cfg(10),                                      # a scene of padding rows only
}
MANY_CFG = _cfg(10)


def case_kwargs(name):
    """the keyword arguments of targets() / box_params() for a case"""
    c = MANY_CFG if name == "many" else CASES[name]
    return dict(num_classes=c["num_classes"], voxel_size=VOXEL_SIZE, point_cloud_range=c["point_cloud_range"], stride=STRIDE,
                overlap=OVERLAP, min_radius=MIN_RADIUS, unknown_labels=c["unknown_labels"], unk_mult=c["unk_mult"])


def _random_boxes(rng, n, cfg, lo=0.2, hi=20.0, spread=1.04):
    r = cfg["point_cloud_range"]
    b = np.zeros((n, 10), f32)
    b[:, 0] = rng.uniform(r[0] * spread, r[3] * spread, n)
    b[:, 1] = rng.uniform(r[1] * spread, r[4] * spread, n)
    b[:, 2] = rng.uniform(-3, 1, n)
    b[:, 3:6] = np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 3)))
    b[:, 6] = rng.uniform(-3.2, 3.2, n)
    b[:, 7:9] = rng.normal(0, 2, (n, 2))
    b[:, 9] = rng.integers(1, cfg["num_classes"] + 1, n)
    return b


def case_boxes(name):
    """(B, M, 10) f32: x y z dx dy dz heading vx vy label (1-based; 0 in padding rows)"""
    cfg = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "a":
        out = np.zeros((2, 80, 10), f32)
        for b in range(2):
            rows = np.sort(rng.choice(80, 60 + b, replace=False))
            out[b, rows] = _random_boxes(rng, rows.size, cfg)
        return out
    if name == "b":
        cell = VOXEL_SIZE[0] * STRIDE
        r0 = cfg["point_cloud_range"][0]
        at = lambda c: r0 + (c + 0.5) * cell                       # the centre of cell c
        line = list(range(-10, 3)) + list(range(177, 191))
        rows = []
        for side in (0.5, 9.0):                                    # radius 2 (the minimum) and radius 6
            rows += [(at(c), at(90), side) for c in line] + [(at(90), at(c), side) for c in line]
            rows += [(at(cx), at(cy), side) for cx in (-1, 0, 179, 180) for cy in (-1, 0, 179, 180)]
        rows.append((r0 - 0.5 * cell, r0 + 0.25 * cell, 4.0))      # (-0.5, 0.25) cells: truncates to (0, 0)
        rows.append((r0 - 0.99 * cell, r0 - 0.01 * cell, 0.5))
        out = np.zeros((1, len(rows), 10), f32)
        for i, (x, y, side) in enumerate(rows):
            out[0, i] = [x, y, 0, side, side * 0.9, 1.5, 0.3, 0, 0, 1 + i % 3]
        return out
    if name in ("c1", "c2"):
        return _random_boxes(rng, 120, cfg)[None]
    if name == "d":
        b = _random_boxes(rng, 712, cfg, lo=1.0, hi=12.0)
        b[:, 0:2] = rng.uniform(-16, 16, (712, 2))
        b[:, 9] = 1
        b[::60, 9] = 2
        return b[None]
    if name == "e":
        return _random_boxes(rng, 40, cfg)[None]
    if name == "f0":
        return np.zeros((1, 0, 10), f32)
    if name == "f1":
        return np.zeros((1, 5, 10), f32)
    raise KeyError(name)


def many_boxes(n=20000):
    """boxes with sides log-uniform over 0.2 .. 20 m, centres up to 4 % outside the range: what pins the radius arithmetic"""
    b = _random_boxes(np.random.default_rng(2024), n, MANY_CFG)
    b[:, [2, 5, 6, 7, 8]] = 0          # (columns the targets do not read: kept out of the fixture's size)
    return b


def quadrant_offsets(max_radius=40):
    """start of radius r's (r+1, r+1) quadrant in the fixture's weights_quadrants"""
    return np.concatenate([[0], np.cumsum([(r + 1) ** 2 for r in range(max_radius + 1)])])
