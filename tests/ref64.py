"""A plain float64 reference of the sparse convolutions, worked out from COORDINATES (no rulebook of the device or of the C
oracle enters), with an error bound per output element that is derived and not tuned.  A helper module, not a fixture.

Quantities, per output element: S = sum x*w over the terms that exist, A = sum |x|*|w| over the same terms, T = the number of
terms (neighbours present x Cin; for the weight gradient the pairs of the offset).  Inputs are 16-bit values, so every product
is exact in f32 and the only error of the accumulator is that of the additions.

THE BOUND.  An f32 sum of T exact products, added in ANY order, errs by at most gamma * A with

    gamma = (T + 64) * 2^-23

  * T * 2^-23: one unit in the last place per addition (twice the unit roundoff: an adder that TRUNCATES is covered);
  * + 64 * 2^-23: a matrix instruction that aligns its 32 products to the largest exponent before it adds them (each product
    may then lose up to an ulp of the largest, twice over for the two halves of a K step).
Both are ASSUMPTIONS about the adder of the matrix unit; nobody has measured them.  They are generous on purpose: with f32
outputs the kernels reach 0.001 - 0.12 of the bound (the larger figures on rows with a single neighbour, where the epilogue's own
f32 roundings dominate); one lost neighbour lies far outside it (tests/test_ref64.py plants such defects).

The epilogue V = relu?(S * scale + shift + residual) adds |scale| * gamma * A for the scaled accumulator,
4 * 2^-24 * (|S * scale| + |shift| + |residual|) for its f32 operations and, for a 16-bit output, one rounding
u * (|V| + e) (e = the error so far; u = 2^-8 for bf16, 2^-11 for fp16) plus 2^-25 absolute for fp16 subnormals.  ReLU is
1-Lipschitz and adds nothing.

Every input is rounded to the 16-bit type first (round16) and the reference is fed those values; magnitudes below the type's
smallest normal are set to zero, so that the matrix unit's treatment of denormals does not enter."""
import numpy as np
import torch

EPS_ADD = 2.0 ** -23          # one unit in the last place of an f32 addition (assumption 1)
ALIGN_TERMS = 64              # products a matrix instruction may align before adding (assumption 2)
U16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
MIN_NORMAL = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14}
FP16_SUBNORMAL = 2.0 ** -25   # half the spacing of fp16 subnormals


def round16(a, td):
    """f32 array -> the same array rounded to `td` (nearest even), values below td's smallest normal set to zero; f32."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(td).float()
    t[t.abs() < MIN_NORMAL[td]] = 0.0
    return t.numpy()


def _triple(v):
    return [int(v)] * 3 if np.isscalar(v) else [int(x) for x in v]


def key(idx, shape):
    idx = np.asarray(idx).astype(np.int64)
    return ((idx[:, 0] * shape[0] + idx[:, 1]) * shape[1] + idx[:, 2]) * shape[2] + idx[:, 3]


def _lookup(idx, B, shape, pad):
    """padded dense lookup (B, D + 2 pad, H + 2 pad, W + 2 pad) -> row or -1"""
    lut = np.full((B, shape[0] + 2 * pad, shape[1] + 2 * pad, shape[2] + 2 * pad), -1, np.int64)
    lut[idx[:, 0], idx[:, 1] + pad, idx[:, 2] + pad, idx[:, 3] + pad] = np.arange(idx.shape[0])
    return lut


def _offsets(ksize):
    k = _triple(ksize)
    return [(a, b, c) for a in range(k[0]) for b in range(k[1]) for c in range(k[2])]


def neighbours_subm(idx, B, shape, ksize=3):
    """(K, n) int64: the row at coordinate + (offset - ksize // 2), or -1.  Offset k = (kz * kH + ky) * kW + kx."""
    idx = np.asarray(idx).astype(np.int64)
    k = _triple(ksize)
    lut = _lookup(idx, B, shape, 1)
    assert max(k) <= 3
    return np.stack([lut[idx[:, 0], idx[:, 1] + 1 + a - k[0] // 2, idx[:, 2] + 1 + b - k[1] // 2, idx[:, 3] + 1 + c - k[2] // 2]
                     for a, b, c in _offsets(k)])


def out_shape_of(shape, ksize, stride, padding):
    k, s, p = _triple(ksize), _triple(stride), _triple(padding)
    return [(shape[d] + 2 * p[d] - k[d]) // s[d] + 1 for d in range(3)]


def neighbours_strided(idx, B, shape, ksize, stride, padding):
    """Output sites (sorted by coordinate key), the output shape and nbr (K, n_out): the input row at out * stride - padding +
    offset, or -1.  An output site exists where at least one input falls into its window."""
    idx = np.asarray(idx).astype(np.int64)
    k, s, p = _triple(ksize), _triple(stride), _triple(padding)
    osh = out_shape_of(shape, k, s, p)
    keys = []
    for off in _offsets(k):
        num = [idx[:, 1 + d] + p[d] - off[d] for d in range(3)]
        ok = np.ones(idx.shape[0], bool)
        for d in range(3):
            ok &= (num[d] % s[d] == 0) & (num[d] >= 0) & (num[d] // s[d] < osh[d])
        o = np.stack([idx[ok, 0]] + [num[d][ok] // s[d] for d in range(3)], 1)
        keys.append(key(o, osh))
    ks = np.unique(np.concatenate(keys))
    out = np.empty((ks.shape[0], 4), np.int64)
    rem = ks
    for d in (3, 2, 1):
        rem, out[:, d] = np.divmod(rem, osh[d - 1])
    out[:, 0] = rem
    P = max(max(k), max(p))
    lut = _lookup(idx, B, shape, P)
    nbr = np.stack([lut[out[:, 0], out[:, 1] * s[0] - p[0] + a + P, out[:, 2] * s[1] - p[1] + b + P, out[:, 3] * s[2] - p[2] + c + P]
                    for a, b, c in _offsets(k)])
    return out.astype(np.int32), osh, nbr


def match_rows(ref_idx, dev_idx, shape):
    """for each device row the reference row at the same coordinate (the site sets must be equal)"""
    kr, kd = key(ref_idx, shape), key(dev_idx, shape)
    assert kr.shape == kd.shape, ("site counts differ", kr.shape, kd.shape)
    o = np.argsort(kr)
    pos = np.searchsorted(kr[o], kd)
    assert (pos < kr.shape[0]).all() and (kr[o][pos] == kd).all(), "the device's output sites are not the reference's"
    return o[pos]


def transpose_nbr(nbr, n_in):
    """(K, n_out) over output rows -> (K, n_in) over input rows: nbr_t[k, i] = o where nbr[k, o] == i"""
    K = nbr.shape[0]
    t = np.full((K, n_in), -1, np.int64)
    for k in range(K):
        o = np.nonzero(nbr[k] >= 0)[0]
        t[k, nbr[k, o]] = o
    return t


def pairs_of(nbr):
    """{(k, in, out)} of a (K, n) neighbour table"""
    k, o = np.nonzero(nbr >= 0)
    return set(zip(k.tolist(), nbr[k, o].tolist(), o.tolist()))


class Sums:
    """S, A (float64 tensors) and T (per row, or per offset for a weight gradient: broadcasts against S)"""

    def __init__(self, S, A, T):
        self.S, self.A, self.T = S, A, T


def conv(x, w, nbr):
    """x (n_in, Cin), w (K, Cout, Cin) (the packed layout), nbr (K, n_out) -> Sums over (n_out, Cout)"""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    w = torch.as_tensor(np.asarray(w), dtype=torch.float64)
    K, Cout, Cin = w.shape
    n_out = nbr.shape[1]
    xa = x.abs()
    S = torch.zeros((n_out, Cout), dtype=torch.float64)
    A = torch.zeros((n_out, Cout), dtype=torch.float64)
    T = torch.zeros((n_out, 1), dtype=torch.float64)
    for k in range(K):
        o = torch.from_numpy(np.nonzero(nbr[k] >= 0)[0])
        if o.numel() == 0:
            continue
        i = torch.from_numpy(np.ascontiguousarray(nbr[k][o.numpy()]))
        S.index_add_(0, o, x[i] @ w[k].T)
        A.index_add_(0, o, xa[i] @ w[k].abs().T)
        T[o] += Cin
    return Sums(S, A, T)


def dgrad(dy, w, nbr, n_in):
    """dx (n_in, Cin) = sum over the transposed pairs of W_k^T dy[o]"""
    w = np.asarray(w)
    return conv(dy, np.ascontiguousarray(w.transpose(0, 2, 1)), transpose_nbr(nbr, n_in))


def wgrad(x, dy, nbr):
    """dW (K, Cout, Cin) = sum over the pairs of offset k of dy[o] (x) x[nbr[k, o]]; T (K, 1, 1) = pairs of the offset"""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    dy = torch.as_tensor(np.asarray(dy), dtype=torch.float64)
    K = nbr.shape[0]
    S = torch.zeros((K, dy.shape[1], x.shape[1]), dtype=torch.float64)
    A = torch.zeros_like(S)
    T = torch.zeros((K, 1, 1), dtype=torch.float64)
    for k in range(K):
        o = np.nonzero(nbr[k] >= 0)[0]
        if o.shape[0] == 0:
            continue
        i = torch.from_numpy(np.ascontiguousarray(nbr[k][o]))
        o = torch.from_numpy(o)
        S[k] = dy[o].T @ x[i]
        A[k] = dy[o].abs().T @ x[i].abs()
        T[k] = o.numel()
    return Sums(S, A, T)


def gamma(T):
    return (T + ALIGN_TERMS) * EPS_ADD


def epilogue(sums, scale=None, shift=None, residual=None, relu=False, out_dtype=torch.float32):
    """(V, bound) float64 tensors: V = relu?(S * scale + shift + residual) and the derived bound of the module docstring.
    residual: what the kernel adds behind the scale (for the split kernels: f32 residual + 16-bit addend, summed here)."""
    S, A = sums.S, sums.A
    f = lambda v: None if v is None else torch.as_tensor(np.asarray(v), dtype=torch.float64)
    scale, shift, residual = f(scale), f(shift), f(residual)
    sc = scale if scale is not None else torch.ones((), dtype=torch.float64)
    V = S * sc
    mag = V.abs()
    if shift is not None:
        V = V + shift
        mag = mag + shift.abs()
    if residual is not None:
        V = V + residual
        mag = mag + residual.abs()
    e = sc.abs() * gamma(sums.T) * A + 4 * 2.0 ** -24 * mag
    if relu:
        V = V.clamp_min(0.0)
    if out_dtype != torch.float32:
        e = e + U16[out_dtype] * (V.abs() + e)
        if out_dtype == torch.float16:
            e = e + FP16_SUBNORMAL
    return V, e


class OutOfBound(AssertionError):
    pass


def check(got, V, bound, n=None, tile=None):
    """-> (worst err / bound, report or None).  No exceptions: every element of every row below n must lie within its own
    bound (a NaN is outside every bound)."""
    if isinstance(got, torch.Tensor):
        got = got.detach().to("cpu")
        got = got.to(torch.float64)
    else:
        got = torch.as_tensor(np.asarray(got), dtype=torch.float64)
    V, bound = torch.as_tensor(V), torch.as_tensor(bound)
    if n is None:
        n = V.shape[0]
    got, V, bound = got[:n], V[:n], bound[:n].expand_as(V[:n])
    assert got.shape == V.shape, (got.shape, V.shape)
    err = (got - V).abs()
    inside = err <= bound          # (False for NaN)
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if bool(inside.all()):
        return worst, None
    bad_rows = torch.nonzero((~inside).reshape(inside.shape[0], -1).any(1)).reshape(-1).numpy()
    rep = [f"{bad_rows.shape[0]} of {inside.shape[0]} rows ({int((~inside).sum())} elements) outside the bound, worst err / bound {worst:.3g}",
           f"first rows {bad_rows[:12].tolist()}, last {bad_rows[-4:].tolist()}",
           f"rows mod 16: {np.bincount(bad_rows % 16, minlength=16).tolist()}"]
    if tile:
        m = np.bincount(bad_rows % tile // 16, minlength=tile // 16)
        rep.append(f"16-row block within the {tile}-row tile: {m.tolist()}; tiles touched: {np.unique(bad_rows // tile).shape[0]}")
    rep.append(f"NaN elements: {int(torch.isnan(got).sum())}")
    return worst, "\n".join(rep)


def assert_within(got, V, bound, n=None, tile=None, what=""):
    """Every element of every row below n within its own bound, or OutOfBound with the rows at fault (count, their indices
    modulo 16 and modulo the tile, the worst ratio).  Returns the largest err / bound of the case."""
    worst, rep = check(got, V, bound, n, tile)
    if rep is not None:
        raise OutOfBound(f"{what}: {rep}")
    return worst


def draw(rng, rows_in, rows_out, Cin, Cout, ksize, td):
    """The inputs of the at-scale tests, as f32 arrays already rounded to `td` (scale and shift stay f32): features x, weight w
    in the module layout (Cout, kD, kH, kW, Cin) and wp = the same values packed (K, Cout, Cin), BatchNorm scale / shift,
    residual res and output gradient dy."""
    k = _triple(ksize)
    w = round16((rng.standard_normal((Cout, *k, Cin)) * 0.05).astype(np.float32), td)
    d = dict(x=round16(rng.standard_normal((rows_in, Cin)).astype(np.float32), td), w=w,
             wp=np.ascontiguousarray(w.reshape(Cout, k[0] * k[1] * k[2], Cin).transpose(1, 0, 2)),
             sc=rng.uniform(0.5, 1.5, Cout).astype(np.float32), sh=rng.standard_normal(Cout).astype(np.float32),
             res=round16(rng.standard_normal((rows_out, Cout)).astype(np.float32), td),
             dy=round16(rng.standard_normal((rows_out, Cout)).astype(np.float32), td))
    return d


def draw_exact(rng, rows_in, rows_out, Cin, Cout, td):
    """x and dy as small integers (-2 .. 2, exact in bf16 and fp16): every product and every partial sum of up to 2^22 of them is
    an integer below 2^24, so an f32 accumulator adds them EXACTLY in any order and the bound of such a case is zero."""
    del td
    return dict(x=rng.integers(-2, 3, (rows_in, Cin)).astype(np.float32), dy=rng.integers(-2, 3, (rows_out, Cout)).astype(np.float32))
