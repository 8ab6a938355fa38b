"""The first BaseBEVBackbone block on sparse rows (findnpropagate_amd/backbones_2d/base_bev_backbone.py) restated on the CPU: the
site sets of the at-scale cases, the BatchNorm2d(eval) fold, the (2, 3, 3) weight of the docstring, the float64 reference of the
output rows with the DERIVED bound of tests/ref64.py (16-bit rows) / tests/ref32.py (f32 rows), an independent dense route through
torch's float64 conv2d, the tile geometry of the dense writer (csrc/dense.hip), and the checks the GPU tests apply — kept here so
that tests/test_ref_bev.py can plant defects and see them rejected without a device.  A helper module, not a fixture; nothing of
the device library is imported.

WHAT IS CHECKED (check_dense).  For a (B, Cout, H, W) f32 map and the reference's output sites with (V, e) per row:
  * dense[b, :, y, x] of every output site lies within its own bound e of V (ref64.check: no allowance, no skipped element);
  * every other cell holds max(shift, 0) of the f32 fold BIT FOR BIT (compared as int32).
No constant here was set by looking at a result of the device."""
import numpy as np
import torch

import ref32 as R32
import ref64 as R

F32 = torch.float32
KSIZE = lambda D: (int(D), 3, 3)
STRIDE, PAD = 1, (0, 1, 1)
K_SLOTS = 64                       # csrc/dense.hip kSlots: occupied cells of a tile that fit the LDS rows
TINY_WEIGHT = 2.0 ** -13           # module weights below this are set to zero (see stable_weight)


def cap_out_of(n, B, H, W):
    """first_block_from_sparse: the a-priori bound on the output sites of a stride-1 3 x 3 window"""
    return max(1, min(9 * max(int(n), 1), B * H * W))


# ------------------------------------------------------------------------------------------------ site sets
def clustered(rng, B, shape, n, spread=4):
    """the clustered generator of tests/test_gpu_bev.py (`_encoded`): six blobs per scene around common centres, clipped at the
    map borders, plus four corner sites; unique rows in random order.  spread: the blobs' standard deviation in cells (4 there)"""
    D, H, W = shape
    cy, cx = rng.integers(0, H, 6), rng.integers(0, W, 6)
    pts = []
    for b in range(B):
        yy = np.clip((cy[:, None] + rng.normal(0, spread, (6, n // (6 * B) + 1))).astype(int), 0, H - 1).ravel()
        xx = np.clip((cx[:, None] + rng.normal(0, spread, (6, n // (6 * B) + 1))).astype(int), 0, W - 1).ravel()
        zz = rng.integers(0, D, yy.shape[0])
        pts.append(np.stack([np.full_like(yy, b), zz, yy, xx], 1))
    idx = np.unique(np.concatenate(pts), axis=0)
    corners = np.array([[0, 0, 0, 0], [0, D - 1, H - 1, W - 1], [B - 1, 0, 0, W - 1], [B - 1, D - 1, H - 1, 0]])
    idx = np.unique(np.concatenate([idx, corners]), axis=0)
    return idx[rng.permutation(idx.shape[0])].astype(np.int32)


def _corner(rng):
    return np.array([[0, 1, 0, 0], [0, 0, 23, 23]], np.int32)


def _d1_odd(rng):
    return clustered(rng, 2, (1, 37, 41), 300)


def _isolated(rng):
    """interior sites on a lattice of pitch 3, one z each: the 3 x 3 windows of the outputs do not overlap"""
    yy, xx = np.meshgrid(np.arange(1, 39, 3), np.arange(1, 39, 3), indexing="ij")
    idx = np.concatenate([np.stack([np.full(yy.size, b), rng.integers(0, 2, yy.size), yy.ravel(), xx.ravel()], 1) for b in range(2)])
    return idx[rng.permutation(idx.shape[0])].astype(np.int32)


def _solid(rng):
    yy, xx = np.meshgrid(np.arange(48), np.arange(48), indexing="ij")
    z0 = np.stack([np.zeros(yy.size, np.int64), np.zeros(yy.size, np.int64), yy.ravel(), xx.ravel()], 1)
    z1 = z0[::3].copy()
    z1[:, 1] = 1
    idx = np.concatenate([z0, z1])
    return idx[rng.permutation(idx.shape[0])].astype(np.int32)


def _mid(rng):
    """about 9 000 rows.  Blobs of spread 4 are under 30 cells wide however many points they get, and a writer tile is a run of 128
    cells of ONE or two map lines: no tile could then hold more than 64 output sites.  Spread 8 makes blobs that do."""
    return clustered(rng, 2, (2, 180, 180), 14000, spread=8)


FULL_OCCUPANCY = 0.19              # per BEV cell: a (z, y, x) site exists with p, 1 - (1 - p)^2 = 0.19


def _full(rng):
    B, (D, H, W) = CASES["full"][:2]
    p = 1.0 - np.sqrt(1.0 - FULL_OCCUPANCY)
    idx = np.argwhere(rng.random((B, D, H, W)) < p)
    return idx[rng.permutation(idx.shape[0])].astype(np.int32)


CASES = {   # name: (B, (D, H, W), generator, seed)
    "corner": (1, (2, 24, 24), _corner, 1),
    "d1-odd": (2, (1, 37, 41), _d1_odd, 2),
    "isolated": (2, (2, 40, 40), _isolated, 3),
    "solid": (1, (2, 48, 48), _solid, 4),
    "mid": (2, (2, 180, 180), _mid, 5),
    "full": (8, (2, 180, 180), _full, 6),
}
_SITES, _TABLES = {}, {}


def sites(name):
    """(idx (n, 4) int32 [b, z, y, x] in the case's row order, B, (D, H, W)); cached per process"""
    if name not in _SITES:
        B, shape, gen, seed = CASES[name]
        idx = np.ascontiguousarray(gen(np.random.default_rng(seed)))
        assert np.unique(idx, axis=0).shape[0] == idx.shape[0]
        _SITES[name] = idx
    B, shape = CASES[name][:2]
    return _SITES[name], B, shape


def table(name):
    """(output sites sorted by coordinate key (n_out, 4) int32 with z = 0, nbr (K, n_out)) of a case, from ref64; cached"""
    if name not in _TABLES:
        idx, B, shape = sites(name)
        _TABLES[name] = neighbours(idx, B, shape)
    return _TABLES[name]


def neighbours(idx, B, shape):
    out, osh, nbr = R.neighbours_strided(idx, B, list(shape), KSIZE(shape[0]), STRIDE, PAD)
    assert osh == [1, shape[1], shape[2]]
    return out, nbr


def draw_rows(name, td, seed=0):
    """(n, 128) f32 features of a case, rounded to `td` when it is a 16-bit type (ref64.round16); cached sites, fresh values"""
    idx, _, _ = sites(name)
    x = np.random.default_rng(1000 + seed).standard_normal((idx.shape[0], 128)).astype(np.float32)
    return x if td == F32 else R.round16(x, td)


# ------------------------------------------------------------------------------------------------ constants and weight
def _f32(t):
    return t.detach().float().cpu().numpy() if hasattr(t, "detach") else np.asarray(t, np.float32)


class Fold:
    """scale, shift, background (f32 arrays: _prepare's operations one for one) and scale64, shift64, background64 (the same fold
    in float64), bias_mag = |bias| + |mean * scale| in float64 (what the error of shift is measured against)"""


def folded(bn):
    """BatchNorm2d(eval) -> Fold.  bn: anything with weight, bias, running_mean, running_var, eps"""
    g, b, m, v = _f32(bn.weight), _f32(bn.bias), _f32(bn.running_mean), _f32(bn.running_var)
    f = Fold()
    inv = np.float32(1.0) / np.sqrt(v + np.float32(bn.eps))
    f.scale = g * inv
    f.shift = b - m * f.scale
    f.background = np.maximum(f.shift, np.float32(0.0))
    assert f.scale.dtype == f.shift.dtype == f.background.dtype == np.float32
    g, b, m, v = (a.astype(np.float64) for a in (g, b, m, v))
    f.scale64 = g / np.sqrt(v + float(bn.eps))
    f.shift64 = b - m * f.scale64
    f.background64 = np.maximum(f.shift64, 0.0)
    f.bias_mag = np.abs(b) + np.abs(m * f.scale64)
    return f


def stable_weight(w2d):
    """the f32 module weight with every magnitude below 2^-13 set to zero: what is left rounds to a NORMAL number of bf16 and of
    fp16 (smallest normal 2^-14), so that ref64.round16 — which sets subnormals to zero to keep the matrix unit's treatment of them
    out of the comparison — and a plain cast to the type give the same bits"""
    w = np.array(_f32(w2d), np.float32)
    w[np.abs(w) < TINY_WEIGHT] = 0.0
    return w


def weight3d(w2d, D):
    """Conv2d weight (Cout, C * D, 3, 3) -> packed (K = D * 9, Cout, C) f32, k = (z * 3 + ky) * 3 + kx:
    W3d[co, z, ky, kx, c] = W2d[co, c * D + z, ky, kx] (height_compression.py's view puts channel c of plane z at c * D + z)"""
    w2d = _f32(w2d)
    Cout, CD = w2d.shape[:2]
    C = CD // D
    assert C * D == CD and w2d.shape[2:] == (3, 3)
    wp = np.empty((D * 9, Cout, C), np.float32)
    for z in range(D):
        for ky in range(3):
            for kx in range(3):
                wp[(z * 3 + ky) * 3 + kx] = w2d[:, z::D, ky, kx][:, :C]
    return wp


def unpermute(w):
    """a (K, Cout, Cin) f32 weight stored with every 16-channel group transposed 4 x 4 (position 4q + r <- channel 4r + q), back
    in plain channel order"""
    K, Cout, Cin = w.shape
    return np.ascontiguousarray(np.asarray(w).reshape(K, Cout, Cin // 16, 4, 4).transpose(0, 1, 2, 4, 3)).reshape(K, Cout, Cin)


# ------------------------------------------------------------------------------------------------ the reference of the rows
def rows_reference(idx, feats, B, shape, w_packed, scale, shift, td, tab=None):
    """-> (output sites (n_out, 4) int32, V, e): V = relu(conv * scale + shift) in float64 on every output site of the (D, 3, 3)
    stride-1 pad-(0, 1, 1) convolution and the bound e of an f32 output.  td f32: the inputs as they are, ref32's bound; a 16-bit
    td: features and weight rounded to it first (ref64.round16), ref64's bound.  tab: (sites, nbr) of neighbours(), if at hand"""
    out, nbr = tab if tab is not None else neighbours(idx, B, shape)
    x, w = np.asarray(feats, np.float32), np.asarray(w_packed, np.float32)
    if td != F32:
        x, w = R.round16(x, td), R.round16(w, td)
    sums = R.conv(x, w, nbr)
    V, e = (R32 if td == F32 else R).epilogue(sums, scale, shift, relu=True, out_dtype=F32)
    return out, V, e


def dense_reference(idx, feats, B, shape, w2d, bn):
    """(B, Cout, H, W) float64 by another route: the (B, C * D, H, W) map as height_compression.py views the dense tensor, zero pad,
    torch's conv2d, BatchNorm2d(eval) and ReLU, all in float64 on the CPU.  Shares no code with rows_reference; small maps only."""
    D, H, W = shape
    idx = np.asarray(idx).astype(np.int64)
    x = torch.as_tensor(np.asarray(feats), dtype=torch.float64)
    C = x.shape[1]
    m = torch.zeros((B, C, D, H, W), dtype=torch.float64)
    m[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]] = x
    m = m.view(B, C * D, H, W)
    w = torch.as_tensor(np.asarray(_f32(w2d)), dtype=torch.float64)
    y = torch.nn.functional.conv2d(torch.nn.functional.pad(m, (1, 1, 1, 1)), w)
    g, b, mean, var = (torch.as_tensor(_f32(a), dtype=torch.float64).view(1, -1, 1, 1) for a in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
    return torch.relu((y - mean) / torch.sqrt(var + float(bn.eps)) * g + b)


def scatter(out, V, background, B, H, W):
    """rows on their sites, `background` (Cout,) everywhere else -> (B, Cout, H, W) of V's dtype"""
    V = np.asarray(V)
    d = np.empty((B, V.shape[1], H, W), V.dtype)
    d[:] = np.asarray(background, V.dtype).reshape(1, -1, 1, 1)
    d[out[:, 0], :, out[:, 2], out[:, 3]] = V
    return d


# ------------------------------------------------------------------------------------------------ the writer's geometry
def tile_cells(H, W):
    """cells of a writer tile for f32 rows: lanes hold 2 cells (8-byte stores) when the plane is even, else 1"""
    return 128 if (H * W) % 2 == 0 else 64


def tile_classes(out_sites, B, H, W):
    """-> dict(empty, slots, over: tiles with 0, 1 .. 64 and more than 64 occupied cells; partial: the plane's last tile is cut;
    tile: cells per tile).  Tiles are runs of consecutive cells of one scene's plane."""
    t, plane = tile_cells(H, W), H * W
    per = -(-plane // t)
    o = np.asarray(out_sites).astype(np.int64)
    cnt = np.bincount(o[:, 0] * per + (o[:, 2] * W + o[:, 3]) // t, minlength=B * per)
    assert cnt.shape[0] == B * per
    return dict(empty=int((cnt == 0).sum()), slots=int(((cnt > 0) & (cnt <= K_SLOTS)).sum()), over=int((cnt > K_SLOTS).sum()),
                partial=plane % t != 0, tile=t)


# ------------------------------------------------------------------------------------------------ the checks
def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def check_dense(dense, out, V, e, background, tile=384):
    """dense (B, Cout, H, W) f32 (numpy) against the reference: -> (worst err / bound over the rows, list of findings; empty:
    the map is right).  See the module docstring."""
    dense = np.asarray(dense)
    B, C, H, W = dense.shape
    fail = []
    if dense.dtype != np.float32:
        return float("inf"), [f"dtype {dense.dtype}, want float32"]
    rows = dense[out[:, 0], :, out[:, 2], out[:, 3]]
    worst, rep = R.check(rows, V, e, None, tile)
    if rep is not None:
        fail.append("rows: " + rep)
    site = np.zeros((B, H, W), bool)
    site[out[:, 0], out[:, 2], out[:, 3]] = True
    assert int(site.sum()) == out.shape[0]
    bg = _bits(background).reshape(1, C, 1, 1)
    bad = (_bits(dense) != bg).any(1) & ~site
    if bad.any():
        cells = np.argwhere(bad)
        fail.append(f"background: {cells.shape[0]} of {int((~site).sum())} cells without a row differ from max(shift, 0) in their bits, "
                    f"first (b, y, x) {cells[:6].tolist()}")
    return worst, fail


def evaluate32(feats, w_packed, nbr, scale, shift):
    """an f32 evaluation of the rows for the planted-defect tests: f32 products summed offset by offset in f32 (for 16-bit values
    the products are exact and ref64's bound covers any order of the additions), f32 epilogue"""
    x, w = np.asarray(feats, np.float32), np.asarray(w_packed, np.float32)
    acc = np.zeros((nbr.shape[1], w.shape[1]), np.float32)
    for k in range(nbr.shape[0]):
        o = np.nonzero(nbr[k] >= 0)[0]
        if o.shape[0]:
            acc[o] += x[nbr[k, o]] @ w[k].T
    return np.maximum(acc * np.asarray(scale, np.float32) + np.asarray(shift, np.float32), np.float32(0.0))


def evaluate_once_rounded(feats, w_packed, nbr, scale, shift):
    """the rows summed in float64 and rounded to f32 once behind the sum and once behind each epilogue step: inside ref32's bound
    for any inputs"""
    s = R.conv(feats, w_packed, nbr).S.numpy().astype(np.float32)
    return np.maximum(s * np.asarray(scale, np.float32) + np.asarray(shift, np.float32), np.float32(0.0))
