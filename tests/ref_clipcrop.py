"""Float64 restatement of the CLIP-crop scoring geometry (csrc/clipcrop.hip), with a forward error
bound carried beside every value, and the case generators shared by tests/test_clipcrop_ref.py (CPU) and
tests/test_gpu_clipcrop.py (GPU).  numpy only.

PLAN.  boxes_to_corners_3d -> un-augment -> lidar2image -> clamp depth to [1e-5, 1e5] -> divide -> img_aug -> truncate ->
on-image test -> clipped box -> side = max(w, h) -> side >= 64, from the f32 numbers the kernel reads.  A quantity is a
pair (v, e): v the f64 value of the exact expression, e a bound on |f32 result - v| for ANY f32 evaluation of it:
  * one f32 operation adds half a spacing of its result, at most U = 2^-24 times the largest magnitude the result can
    have, and carries its operands' bounds through (first and second order);
  * a k-term dot product is bounded independently of the summation order and of fusing: every product passes through
    at most k roundings, so the rounding part is ((1 + U)^k - 1) * sum |a_i| |b_i| (magnitudes taken at their upper
    ends).  The reference's matmul and the kernel's left-to-right sum (built with -ffp-contract=off) both fit;
  * cosf / sinf are allowed TRIG_ULP spacings of their result.  The HIP math accuracy table is not among the ROCm
    documents at hand, so 4 ulp is ASSUMED, not measured;
  * the clamp maps the ends of the interval; the division divides by the lower end of |depth|.
The outcome per (box, camera) is a SET of admissible results: each corner's pixel lies in [trunc(v - e), trunc(v + e)],
hence ranges for xmin, xmax, ymin, ymax, and after clipping for x1, y1, x2, y2 and side.  cam_mask is surely 1 if some
corner is surely on the image with depth surely >= 0.01f, surely 0 if no corner can be, else open.  A pair is DECIDED
when its output is a single value: mask surely 0; or mask surely 1 with the crop surely too small; or mask surely 1
with x1, y1, x2, y2 single.

SAMPLE.  Bilinear sampling with zero padding at unit[j] * side + x1, normalised by W (H) and un-normalised with
align_corners = False, all in f64, from the f32 unit table, the rectangle and the stored image values.  Bound per
element: (position error of the f32 chain gx -> ix, one half-spacing per operation) x (largest difference between
adjacent taps in the 3 x 3 cells around the sample, taps off the image counting 0) + the rounding of the weights, the
four weighted products and the three additions; for f16 output half an f16 spacing of the result and half the f16
subnormal spacing on top."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149          # f32 subnormal spacing: covers a result that is not normal
TRIG_ULP = 4.0              # assumed (see above)
IMAGE_ORDER = [2, 0, 1, 5, 3, 4]


# ------------------------------------------------------------------------------------------ (value, bound) arithmetic
def _c(x):
    return np.asarray(x, np.float64), 0.0


def _hi(a):
    return np.abs(a[0]) + a[1]


def _dot(*terms):
    """sum a_i * b_i of (v, e) pairs; any order, fused or not."""
    v, prop, mag = 0.0, 0.0, 0.0
    for a, b in terms:
        v = v + a[0] * b[0]
        prop = prop + np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + a[1] * b[1]
        mag = mag + _hi(a) * _hi(b)
    return v, prop + ((1.0 + U) ** len(terms) - 1.0) * mag + TINY


def _add(a, b, sign=1.0):
    v = a[0] + sign * b[0]
    e = a[1] + b[1]
    return v, e + U * (np.abs(v) + e) + TINY


def _mul(a, b):
    return _dot((a, b))


def _div(a, b):
    """a / b with b's interval away from 0."""
    lo = np.abs(b[0]) - b[1]
    assert np.all(lo > 0)
    v = a[0] / b[0]
    e = (a[1] + np.abs(v) * b[1]) / lo
    return v, e + U * (np.abs(v) + e) + TINY


def _trig(x32):
    x = x32.astype(np.float64)
    out = []
    for f in (np.cos, np.sin):
        v = f(x)
        out.append((v, TRIG_ULP * 2.0 * U * np.abs(v) + TINY))
    return out


# ------------------------------------------------------------------------------------------ plan
TEMPLATE = np.array([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]], np.float64) / 2


def project(boxes, rinv, trans, l2i, iaug):
    """(rx, ry, rz, qz_raw): (v, e) pairs of shape (n, 6, 8), and the unclamped depth."""
    for a in (boxes, rinv, trans, l2i, iaug):
        assert a.dtype == np.float32
    bx = boxes.astype(np.float64)[:, None, :]                        # (n, 1, 7)
    cs, sn = _trig(boxes[:, 6][:, None])
    lx, ly, lz = (_c(bx[:, :, 3 + d] * TEMPLATE[None, :, d]) for d in range(3))     # (n, 8), exact: dims times +-1/2
    zero = _c(np.zeros_like(lx[0]))
    nsn = (-sn[0], sn[1])
    # rotate about z as a three-term product with the matrix's 0 / 1 entries (box_utils.py:28-53), then + centre
    px = _add(_dot((lx, cs), (ly, nsn), (lz, zero)), _c(bx[:, :, 0]))
    py = _add(_dot((lx, sn), (ly, cs), (lz, zero)), _c(bx[:, :, 1]))
    pz = _add(lz, _c(bx[:, :, 2]))
    p = [_add(q, _c(np.float64(trans[d])), -1.0) for d, q in enumerate((px, py, pz))]
    R = rinv.astype(np.float64)
    u = [_dot(*[(_c(R[r, d]), p[d]) for d in range(3)]) for r in range(3)]
    u = [(v[:, None, :], e[:, None, :]) for v, e in u]               # (n, 1, 8)
    L = l2i.astype(np.float64)[None, :, :, :, None]                  # (1, 6, 4, 4, 1)
    q = [_add(_dot(*[(_c(L[:, :, r, d]), u[d]) for d in range(3)]), _c(L[:, :, r, 3])) for r in range(3)]   # (n, 6, 8)
    qz_raw = q[2]
    lo = np.clip(qz_raw[0] - qz_raw[1], np.float64(np.float32(1e-5)), np.float64(np.float32(1e5)))
    hi = np.clip(qz_raw[0] + qz_raw[1], np.float64(np.float32(1e-5)), np.float64(np.float32(1e5)))
    qz = ((lo + hi) / 2, (hi - lo) / 2)
    qx, qy = _div(q[0], qz), _div(q[1], qz)
    A = iaug.astype(np.float64)[None, :, :, :, None]
    r = [_add(_dot((_c(A[:, :, k, 0]), qx), (_c(A[:, :, k, 1]), qy), (_c(A[:, :, k, 2]), qz)), _c(A[:, :, k, 3])) for k in range(3)]
    return r[0], r[1], r[2], qz_raw


def _trunc_range(x):
    return np.trunc(x[0] - x[1]).astype(np.int64), np.trunc(x[0] + x[1]).astype(np.int64)


def plan(boxes, rinv, trans, l2i, iaug, H, W, min_crop=64, exact=False):
    """Admissible results per (box, camera); every array (n, 6), ranges as (lo, hi) int64.  exact: the bounds are taken as 0,
    for inputs on which every f32 operation is exact (the tests show that it is before they use this)."""
    rx, ry, rz, _ = project(boxes, rinv, trans, l2i, iaug)
    if exact:
        rx, ry, rz = ((v, 0.0 * e) for v, e in (rx, ry, rz))
    xl, xh = _trunc_range(rx)
    yl, yh = _trunc_range(ry)
    near = np.float64(np.float32(0.01))
    sure = (xl >= 0) & (xh < W) & (yl >= 0) & (yh < H) & (rz[0] - rz[1] >= near)
    maybe = (xh >= 0) & (xl < W) & (yh >= 0) & (yl < H) & (rz[0] + rz[1] >= near)
    mask_lo, mask_hi = sure.any(-1), maybe.any(-1)
    rng = {}
    for name, lo, hi, size in (("x", xl, xh, W), ("y", yl, yh, H)):
        rng[name + "1"] = (np.clip(lo.min(-1), 0, size), np.clip(hi.min(-1), 0, size))
        rng[name + "2"] = (np.clip(lo.max(-1), 0, size), np.clip(hi.max(-1), 0, size))
    single = np.ones_like(mask_lo)
    for lo, hi in rng.values():
        single &= lo == hi
    side_lo = np.maximum(np.maximum(rng["x2"][0] - rng["x1"][1], rng["y2"][0] - rng["y1"][1]), 0)
    side_hi = np.maximum(rng["x2"][1] - rng["x1"][0], rng["y2"][1] - rng["y1"][0])
    decided = ~mask_hi | (mask_lo & ((side_hi < min_crop) | single))
    side = np.maximum(rng["x2"][0] - rng["x1"][0], rng["y2"][0] - rng["y1"][0])           # meaningful where single
    valid = mask_lo & single & (side >= min_crop)
    rect = np.zeros(mask_lo.shape + (4,), np.float32)
    rect[valid] = np.stack([rng["x1"][0], rng["y1"][0], side, np.ones_like(side)], -1)[valid]
    return dict(mask_lo=mask_lo, mask_hi=mask_hi, decided=decided, rect=rect, mask=mask_lo.astype(np.uint8), valid=valid,
                side_lo=side_lo, side_hi=side_hi, min_crop=min_crop, **rng)


def check_plan(p, rect, mask):
    """Device rect (n, 6, 4) f32 / mask (n, 6) u8 against the admissible sets.  Returns the list of violations."""
    bad = []
    if not np.all(np.isfinite(rect)) or not np.all(mask <= 1):
        return ["an element was not written"]
    d = p["decided"]
    for i, c in zip(*np.nonzero(d & ((mask != p["mask"]) | (rect != p["rect"]).any(-1)))):
        bad.append(f"decided pair ({i},{c}): got mask {mask[i, c]} rect {rect[i, c].tolist()}, want {p['mask'][i, c]} {p['rect'][i, c].tolist()}")
    for i, c in zip(*np.nonzero(~d)):
        why = pair_violation(p, i, c, int(mask[i, c]), rect[i, c].astype(np.float64))
        if why:
            bad.append(f"undecided pair ({i},{c}): {why}: mask {mask[i, c]} rect {rect[i, c].tolist()}")
    return bad


def pair_violation(p, i, c, m, r):
    """None if mask m and rect r (4 numbers) are admissible for pair (i, c), else the reason."""
    if m == 0:
        if p["mask_lo"][i, c] or np.any(r):
            return "mask 0 not admissible, or a rectangle without a camera"
    elif not p["mask_hi"][i, c]:
        return "mask 1 not admissible"
    elif r[3] == 0:
        if np.any(r) or p["side_lo"][i, c] >= p["min_crop"]:
            return "no crop, but the side is surely large enough"
    else:
        x1, y1, s = r[0], r[1], r[2]
        ok = r[3] == 1 and p["x1"][0][i, c] <= x1 <= p["x1"][1][i, c] and p["y1"][0][i, c] <= y1 <= p["y1"][1][i, c] and s >= p["min_crop"]
        # side = max(x2 - x1, y2 - y1) for some admissible x2, y2: every integer between the two ends is reached
        ok = ok and max(p["x2"][0][i, c] - x1, p["y2"][0][i, c] - y1) <= s <= max(p["x2"][1][i, c] - x1, p["y2"][1][i, c] - y1)
        if not ok:
            return "rectangle outside its ranges"
    return None


def crop_pairs(rect):
    """(M, 2) [box, camera] of the valid crops in the reference's order: cameras in image_order, boxes ascending."""
    out = [(i, c) for c in IMAGE_ORDER for i in range(rect.shape[0]) if rect[i, c, 3] > 0]
    return np.array(out, np.int32).reshape(-1, 2)


def replay_f32(boxes, rinv, trans, l2i, iaug):
    """The kernel's chain in numpy f32, left to right, unfused: (rx, ry, rz) f32 (n, 6, 8).  Not a reference: one f32
    evaluation whose distance from the f64 value is printed against the bound."""
    f = np.float32
    b = boxes[:, None, :]
    cs, sn = np.cos(b[..., 6]).astype(f), np.sin(b[..., 6]).astype(f)
    t = TEMPLATE.astype(f)[None]
    lx, ly, lz = b[..., 3] * t[..., 0], b[..., 4] * t[..., 1], b[..., 5] * t[..., 2]
    p = [lx * cs + ly * (-sn) + b[..., 0] - trans[0], lx * sn + ly * cs + b[..., 1] - trans[1], lz + b[..., 2] - trans[2]]
    u = [(rinv[r, 0] * p[0] + rinv[r, 1] * p[1] + rinv[r, 2] * p[2])[:, None, :] for r in range(3)]
    L, A = l2i[None, :, :, :, None], iaug[None, :, :, :, None]
    q = [L[:, :, r, 0] * u[0] + L[:, :, r, 1] * u[1] + L[:, :, r, 2] * u[2] + L[:, :, r, 3] for r in range(3)]
    qz = np.clip(q[2], f(1e-5), f(1e5))
    qx, qy = q[0] / qz, q[1] / qz
    out = [A[:, :, k, 0] * qx + A[:, :, k, 1] * qy + A[:, :, k, 2] * qz + A[:, :, k, 3] for k in range(3)]
    assert all(o.dtype == f for o in out)
    return out


def worst_ratio(vals, got, keep):
    """max |got - v| / e over the kept corners, for the (v, e) pairs vals and the f32 arrays got."""
    w = 0.0
    for (v, e), g in zip(vals, got):
        r = np.abs(g.astype(np.float64) - v) / e
        if keep.any():
            w = max(w, float(r[keep].max()))
    return w


# ------------------------------------------------------------------------------------------ sample
def unit_table(S):
    """An ascending [0, 1] table of S pixel-centre positions, min-max normalised like the reference's grid, f32."""
    f = np.float32
    g = ((np.arange(S, dtype=f) * f(2) + f(1)) / f(S) - f(1)).astype(f)
    if S == 1:
        return np.zeros(1, f)
    return ((g - g.min()) / (g.max() - g.min())).astype(f)


def _position(unit, side, a1, size):
    """ix (v, e) of the chain  unit * side + a1 -> / size * 2 - 1 -> ((. + 1) * size - 1) / 2."""
    g = _add(_mul(_c(unit), _c(side)), _c(a1))
    d = _div(g, _c(size))
    n = _add((d[0] * 2.0, d[1] * 2.0), _c(1.0), -1.0)           # (* 2 and / 2 are exact)
    p = _add(_mul(_add(n, _c(1.0)), _c(size)), _c(1.0), -1.0)
    return p[0] / 2.0, p[1] / 2.0


class SampleRef:
    """Per camera: the image in f64, zero-padded, and the largest adjacent-tap difference in the 4 x 4 taps (3 x 3 cells) around a cell."""
    PAD = 3

    def __init__(self, images):
        self.images = images                      # (6, C, H, W) f32 or f16 numpy
        self.C, self.H, self.W = images.shape[1:]
        self._cam = {}

    def cam(self, c):
        if c not in self._cam:
            P = self.PAD
            img = np.zeros((self.C, self.H + 2 * P, self.W + 2 * P))
            img[:, P:-P, P:-P] = self.images[c].astype(np.float64)          # f16 upcasts exactly
            d = np.zeros_like(img)                                          # at tap (y, x): differences to its right / lower neighbour
            d[:, :, :-1] = np.abs(img[:, :, 1:] - img[:, :, :-1])
            d[:, :-1, :] = np.maximum(d[:, :-1, :], np.abs(img[:, 1:, :] - img[:, :-1, :]))
            # window of cell (y0, x0): taps y0-1 .. y0+2, x0-1 .. x0+2; stored at [y0, x0] (padded index)
            wx = np.zeros_like(d)
            for s in (-1, 0, 1, 2):
                wx = np.maximum(wx, np.roll(d, -s, axis=2))
            w = np.zeros_like(d)
            for s in (-1, 0, 1, 2):
                w = np.maximum(w, np.roll(wx, -s, axis=1))
            self._cam[c] = (img, w)
        return self._cam[c]

    def crop(self, c, x1, y1, side, unit, f16_out=False):
        """(value, bound), each (C, S, S) f64, of one crop of camera c."""
        img, win = self.cam(c)
        P, H, W = self.PAD, self.H, self.W
        ix, ex = _position(unit, float(side), float(x1), float(W))
        iy, ey = _position(unit, float(side), float(y1), float(H))
        fx, fy = np.floor(ix), np.floor(iy)
        wx1, wy1 = ix - fx, iy - fy
        # cells wholly off the padded image have only zero taps around them: move them to the pad, where that is so too
        cx = np.clip(fx, -2, W).astype(np.int64) + P
        cy = np.clip(fy, -2, H).astype(np.int64) + P
        offx, offy = (fx < -2) | (fx > W), (fy < -2) | (fy > H)
        Y, X = cy[:, None], cx[None, :]
        t00, t01, t10, t11 = img[:, Y, X], img[:, Y, X + 1], img[:, Y + 1, X], img[:, Y + 1, X + 1]
        w00, w01 = ((1 - wx1)[None, :] * (1 - wy1)[:, None]), (wx1[None, :] * (1 - wy1)[:, None])
        w10, w11 = ((1 - wx1)[None, :] * wy1[:, None]), (wx1[None, :] * wy1[:, None])
        off = (offx[None, :] | offy[:, None])[None]
        val = np.where(off, 0.0, t00 * w00 + t01 * w01 + t10 * w10 + t11 * w11)
        mag = np.abs(t00) * w00 + np.abs(t01) * w01 + np.abs(t10) * w10 + np.abs(t11) * w11
        D = win[:, Y, X]
        # (all taps of the window 0: the result is exactly 0 wherever in the window the f32 position falls, and the bound is 0)
        bound = np.where(off | ((D == 0) & (mag == 0)), 0.0, (ex[None, None, :] + ey[None, :, None]) * D + 8 * U * mag + 4 * TINY)
        if f16_out:
            bound = bound + 2.0 ** -11 * (np.abs(val) + bound) + 2.0 ** -25
        return val, bound


# ------------------------------------------------------------------------------------------ cases
def procedural_images(h, w):
    """(6, 3, h, w) f32 in [0, 1]; the images of the golden fixtures."""
    y, x = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    out = np.empty((6, 3, h, w), np.float32)
    for c in range(6):
        for ch in range(3):
            out[c, ch] = 0.5 + 0.5 * np.sin(np.float32(0.013 * (ch + 1)) * x + np.float32(0.7 * c)) * np.cos(np.float32(0.011) * y + np.float32(0.3 * ch))
    return out


def _lidar_aug(kind):
    m = np.eye(4)
    if kind != "none":
        a = 0.35
        m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        m[:3, 3] = [0.7, -0.4, 0.2]
        if kind == "scale":
            m[:3, :3] *= 0.93                       # not orthogonal: the inverse is not the transpose
    return m.astype(np.float32)


def _img_aug(kind, rng):
    out = np.tile(np.eye(4), (6, 1, 1))
    if kind == "256x704":
        for c in range(6):
            s = rng.uniform(0.43, 0.45)
            out[c, :2, :2] = np.diag([s, s])
            out[c, :2, 3] = [rng.uniform(-5, 5), -(900 * s - 256) + rng.uniform(-4, 0)]
            # a general matrix: depth leaks a little into the pixel (A[2], A[6]) and rz is not the depth alone (A[8..11])
            out[c, 0, 2], out[c, 1, 2] = rng.uniform(0.05, 0.2), rng.uniform(-0.2, -0.05)
            out[c, 2, :] = [rng.uniform(-1e-4, 1e-4), rng.uniform(-1e-4, 1e-4), rng.uniform(0.8, 1.2), rng.uniform(-0.5, 0.5)]
        out[1, 0, :] = [-out[1, 0, 0], 0, out[1, 0, 2], 704.0 - out[1, 0, 3]]      # flipped
    return out.astype(np.float32)


PLAN_CASES = [  # name, n, geometry, lidar augmentation, seed
    ("n1_900x1600_none", 1, "900x1600", "none", 11),
    ("n42_256x704_rot", 42, "256x704", "rot", 12),
    ("n43_900x1600_scale", 43, "900x1600", "scale", 13),
    ("n300_256x704_scale", 300, "256x704", "scale", 14),
    ("n300_900x1600_none", 300, "900x1600", "none", 15),
]


def plan_case(name):
    """Inputs of one random plan case: boxes (n, 7), lidar_aug (4, 4), lidar2image and img_aug (6, 4, 4), f32; H, W."""
    from findnpropagate_amd import synthetic as syn
    _, n, geom, aug, seed = next(c for c in PLAN_CASES if c[0] == name)
    rng = np.random.default_rng(seed)
    boxes, _ = syn.make_boxes(rng, n)
    if n == 1:
        boxes[0, :2] = [9.0, 1.5]                   # in front of camera 0, near enough for a crop
    if geom == "256x704":
        boxes[:, :2] *= 0.7                         # at this scale the far boxes fall under the 64 px minimum anyway
    m = _lidar_aug(aug)
    boxes = boxes.astype(np.float32)
    boxes[:, :3] = (boxes[:, :3].astype(np.float64) @ m[:3, :3].astype(np.float64).T + m[:3, 3]).astype(np.float32)
    l2i = syn.make_cameras(1)["lidar2image"][0]
    H, W = (900, 1600) if geom == "900x1600" else (256, 704)
    return dict(name=name, boxes=np.ascontiguousarray(boxes), lidar_aug=m, l2i=np.ascontiguousarray(l2i), iaug=_img_aug(geom, rng), H=H, W=W)


# Exact cases: a dyadic pinhole looking along +x (column = 800 - 512 y / x, row = 450 - 512 z / x), yaw 0, centres and sizes
# multiples of 2^-4, depths powers of two: every f32 operation of the chain is exact, so rect and mask are known integers.
def _pinhole():
    L = np.zeros((6, 4, 4), np.float32)
    L[:, 3, 3] = 1
    L[:, 0, :3], L[:, 1, :3], L[:, 2, :3] = [800, -512, 0], [450, 0, -512], [1, 0, 0]
    return L


def _edge(boxes, expect, W=1600, H=900, iaug=None):
    A = np.tile(np.eye(4, dtype=np.float32), (6, 1, 1)) if iaug is None else np.tile(np.asarray(iaug, np.float32), (6, 1, 1))
    return dict(boxes=np.asarray(boxes, np.float32).reshape(-1, 7), l2i=_pinhole(), iaug=A, H=H, W=W, lidar_aug=np.eye(4, dtype=np.float32),
                expect=expect)


def edge_cases():
    """name -> case; expect = (mask, [x1, y1, side, valid]) of every (box 0, camera): all six cameras share the matrices.
    A box at depth d in {4, 8} (front face at d - 1/2 ... use thin boxes: dx = 0 is allowed, every corner at depth d)."""
    E = {}
    # depth 8, dx = 0: column = 800 - 64 y, row = 450 - 64 z.  y in [-1, 1], z in [-0.5, 0.5] -> columns 736..864, rows 418..482
    E["inside"] = _edge([8, 0, 0, 0, 2, 1, 0], (1, [736, 418, 128, 1]))
    # columns exactly 0 and 64: y = 12.5 and 11.5 (centre 12, dy 1); rows 386..514: side = max(64, 128)
    E["column_0"] = _edge([8, 12, 0, 0, 1, 2, 0], (1, [0, 386, 128, 1]))
    # columns exactly W - 1 = 1599 need 64 y = -799: not dyadic at depth 8; depth 512 gives column = 800 - y
    # y = -799 and -735 (centre -767, dy 64) -> columns 1599, 1535; rows 450 - z: z in [-32, 32] -> 418..482
    E["column_W-1"] = _edge([512, -767, 0, 0, 64, 64, 0], (1, [1535, 418, 64, 1]))
    # columns W = 1600 and 1664: both off the image (ix < W fails), so no camera
    E["column_W"] = _edge([512, -832, 0, 0, 64, 64, 0], (0, [0, 0, 0, 0]))
    # columns W + 1 and W - 63: the far corner is off, the near one on: x2 clips to W, side = W - 1537 = 63 -> rows decide: 64
    E["column_W+1"] = _edge([512, -769, 0, 0, 64, 64, 0], (1, [1537, 418, 64, 1]))
    # columns in (-1, 0): y = 12.5 + 1/128 at depth 8 -> column -0.5: truncates to 0 and counts as on the image, as .long() does.
    # The other corners of that box: y = 13.5 + 1/128 -> column -64.5 -> -64 (off).  rows 386..514
    E["column_-0.5"] = _edge([8, 13 + 1 / 128, 0, 0, 1, 2, 0], (1, [0, 386, 128, 1]))
    # column exactly -1 and beyond: off the image
    E["column_-1"] = _edge([8, 13 + 1 / 64, 0, 0, 1, 2, 0], (0, [0, 0, 0, 0]))
    # rz on both sides of 0.01f: img_aug row 2 = [0, 0, 2^-10, 0] turns depth 8 into 0.0078125 (< 0.01) and depth 16 into 0.015625
    A = np.eye(4)
    A[2, 2] = 2.0 ** -10
    E["rz_below"] = _edge([8, 0, 0, 0, 2, 1, 0], (0, [0, 0, 0, 0]), iaug=A)
    E["rz_above"] = _edge([16, 0, 0, 0, 4, 2, 0], (1, [736, 418, 128, 1]), iaug=A)
    # side exactly 63 and 64 (depth 512: one metre is one pixel)
    E["side_63"] = _edge([512, 0, 0, 0, 63, 63, 0], (1, [0, 0, 0, 0]))
    E["side_64"] = _edge([512, 0.5, 0.5, 0, 63, 64, 0], (1, [768, 417, 64, 1]))     # columns 831 .. 768 (y = -31 .. 32), rows 417.5 -> 417, 481.5 -> 481
    # wholly behind the camera: depth clamps to 1e-5, the coordinates are huge, rz = 1e-5 < 0.01
    E["behind"] = _edge([-8, 0, 0, 0, 2, 1, 0], (0, [0, 0, 0, 0]))
    # straddles the camera plane (x from -4 to 12): the far face is on the image at depth 12 (not dyadic, but a third of a pixel
    # clear of any decision; the restatement must call it decided), the near face has depth 1e-5 and coordinates of order
    # +-1e8 in both directions, which convert and clip to all four borders
    E["straddle"] = _edge([4, 0, 0, 16, 16, 16, 0], (1, [0, 0, 1600, 1]))
    # every corner off the image, the bounding box covers it: no camera, as in the reference
    E["cover"] = _edge([8, 0, 0, 0, 32, 16, 0], (0, [0, 0, 0, 0]))
    # power-of-two scale, integer shift and a depth term in the pixel: column = 0.5 (800 - 64 y) + 0.25 * 8 - 100
    A = np.eye(4)
    A[0, :] = [0.5, 0, 0.25, -100]
    A[1, :] = [0, 0.5, -0.125, -50]
    # columns: y = -1, 1 -> 0.5 * (864, 736) + 2 - 100 = 334, 270; rows: z = -2, 2 -> 0.5 * (578, 322) - 1 - 50 = 238, 110
    E["aug_depth_term"] = _edge([8, 0, 0, 0, 2, 4, 0], (1, [270, 110, 128, 1]), W=704, H=256, iaug=A)
    return E


SAMPLE_RECTS = ["inside", "overhang", "larger", "x1=W", "far_corner"]


def sample_rects(H, W):
    """(5, 4) f32 [x1, y1, side, 1]: wholly inside; overhanging right and bottom; larger than both image dimensions from the
    origin; x1 = W (the sample of column j lies at pixel coordinate W - 0.5 + unit[j] * side, so the first columns still weigh the last
    pixel column in and every column from W + 0.5 on is exactly 0); side 64 ending at the far corner."""
    s_in = min(H, W) // 2
    return np.array([[W // 8, H // 8, s_in, 1], [W - 50, H - 40, 90, 1], [0, 0, max(H, W) + 37, 1], [W, H // 2, 70, 1], [W - 64, H - 64, 64, 1]], np.float32)
