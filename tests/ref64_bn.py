"""A plain float64 reference of BatchNorm1d in training mode fused with the residual add and the ReLU behind it (csrc/bnorm.hip:
fnp_bn_train_forward / fnp_bn_train_backward), written from the formulas in that file's header, with an error bound per output
that is derived and not tuned.  A helper module like tests/ref64.py (whose comparator it is used with), not a fixture.

    forward :  mean_c, var_c over the n valid rows (biased), invstd = 1 / sqrt(var + eps),
               y = act((x - mean) * invstd * gamma + beta [+ residual]),
               running_mean' = (1 - momentum) * running_mean + momentum * mean,
               running_var'  = (1 - momentum) * running_var  + momentum * var * n / (n - 1)      (n == 1: var itself)
    backward:  g = dy * [y > 0]  (relu; else g = dy),  dbeta = sum g,  dgamma = sum g * xhat,  xhat = (x - mean) * invstd,
               dx = gamma * invstd * (g - dbeta / n - xhat * dgamma / n),  dresidual = g

Inputs are the STORED values (x, residual, dy, y already rounded to the feature dtype; gamma, beta, running statistics f32; eps and
momentum rounded to f32, as the C ABI takes them).  The ReLU mask of the backward is `y_stored > 0` on the tensor the kernel is
GIVEN: that is the definition of the operation, so there is no allowance for an element "on the other side" of the ReLU.

Notation: u = 2^-24 (unit roundoff of f32, round to nearest), v = 2^-53 (of f64), n = rows, per channel m = mean, is = invstd,
d = |x - m|, A1 = mean |x|, Ex2 = mean x^2.  All bounds hold for ANY order of the additions.

THE STATISTICS (f64 in the kernel, f64 here; both sides err, both are counted).
  * a sum of n terms in f64, any order: (n - 1) * v * sum |term| to first order for each side, n * 2^-52 * sum |term| for both
    (the second-order remainder is below (n - 1) * 2^-30 of the first and n - 1 -> n pays for it while n < 2^30).  Products x * x
    and g * xhat_f32 of two f32 values are exact in f64.
      E_sum(x) / n = n * 2^-52 * A1
  * mean = sum / n: one division per side,  E_m = n * 2^-52 * A1 + 2^-52 * |m|;  stored as f32:
      B_mean = E_m + u * (|m| + E_m)
  * var = E[x^2] - mean^2 formed in f64 (the kernel's form; this module forms mean (x - m)^2, which errs less):
      E_var = n * 2^-52 * (Ex2 + 2 |m| A1) + 4 * 2^-52 * (Ex2 + m^2)
    (sum of squares; the sum's error through 2 m * delta m; per side the division, the product m * m, the subtraction and the
    division inside m: at most 2 Ex2 + 3 m^2 <= 4 (Ex2 + m^2) times v.)  The error is ABSOLUTE and scales with Ex2 + m^2, not
    with var: with |m| >> std this term is the bound of invstd.  Clamping var at 0 moves it towards the true value.
  * invstd = 1 / sqrt(var + eps): add, sqrt, divide: 2 v relative here, 4.5 v in the kernel if its f64 sqrt and division are only
    good to one ulp (ASSUMED no worse), 8 v = 2^-50 together; |d invstd / d var| = invstd^3 / 2 is largest at the
    smallest variance the error admits, lo = max(var - E_var, 0) + eps:
      E_is = E_var / 2 * lo^-1.5 + 2^-50 * is,      B_invstd = E_is + u * (is + E_is)
  * running statistics: momentum * (E_m resp. E_var * n / (n - 1)) + 2^-50 * (|(1 - momentum) * old| + |momentum * new|) for the f64
    operations of both sides, then one f32 rounding u * (|value| + error so far).

THE FORWARD APPLY (f32 in the kernel), with the STORED mean and invstd off by at most B_mean = Bm and B_invstd = Bi:
      t1 = x - mean_f         error D1 = Bm (1 + u) + u d
      t2 = t1 * invstd_f      error of xhat:  Dxh = (1 + u)^2 * (Bm (is + Bi) + d (Bi + 2 u (is + Bi)))
      t3 = t2 * gamma         D3 = |gamma| Dxh (1 + u) + u |xhat gamma|
      t4 = t3 + beta          D4 = D3 + u' (|xhat gamma + beta| + D3)
      t5 = t4 + residual      D5 = D4 + u' (|V| + D4)                                   (only with a residual)
  Five roundings, each counted where it happens.  The compiler may contract t3 * gamma + beta into one FMA: that omits the
  rounding of t3 and stays inside.  (x - mean) * invstd is an addition feeding a product and cannot be contracted without
  reassociation.  u' = u + 2^-48 pays for this module's own f64 operations.  The term Bm * is * |gamma| is the propagated error of
  the f32-rounded mean: about u |m| / std per unit of gamma, it DOMINATES when |m| >> std.  ReLU is 1-Lipschitz: nothing.

THE BACKWARD.  The mask is exact and g is a stored value or zero, so dresidual = g is exact: bound ZERO.
  * dbeta = sum g:   E = n * 2^-52 * sum |g|,  B_dbeta = E + u (|dbeta| + E)
  * dgamma = sum g * xhat_f32 (xhat computed in f32 inside the sum, error Dxh per element as above, with sum |g| d = Sgx / is):
      E = (1 + u)^2 * (Bm (is + Bi) sum |g| + (Bi + 2 u (is + Bi)) sum |g| d)  +  (n + 8) * 2^-52 * (sum |g xhat| + the first term)
      B_dgamma = E + u (|dgamma| + E)
    It grows like n * u * mean |g xhat| while dgamma itself grows like sqrt(n): at 2 * 10^6 rows the bound is ~1e-4 of dgamma.
  * dx, nine f32 roundings: xhat (2, Dxh), q1 = dbeta_f * inv_n, s1 = g - q1, q2 = xhat_f * dgamma_f, q3 = q2 * inv_n,
    s2 = s1 - q3, p = gamma * invstd_f, dx = p * s2.  inv_n = 1.0f / (float) n: (float) n is exact (ASSUMPTION: n < 2^24) and
    the division is granted 6 u relative — 2.5 ulp, what a division that is not correctly rounded may still be held to; a
    correctly rounded one uses u of it.  With M = |g| + |dbeta| / n + |xhat| |dgamma| / n >= |g - dbeta / n - xhat dgamma / n|:
      Eq1 = Bdb / n (1 + 7u) + 7u |dbeta| / n                       Es1 = Eq1 + u (|g| + |dbeta| / n + Eq1)
      Eq2 = Dxh (|dgamma| + Bdg) (1 + u) + |xhat| (Bdg + u (|dgamma| + Bdg))
      Eq3 = Eq2 / n (1 + 7u) + 7u |xhat| |dgamma| / n              Es2 = Es1 + Eq3 + u (M + Es1 + Eq3)
      Ep  = |gamma| (Bi + u (is + Bi))
      Edx = Ep (M + Es2) + |gamma| is Es2 + u (|gamma| is + Ep) (M + Es2)  +  2^-48 |gamma| is M
    g - q1 and s1 - q3 may each be contracted into an FMA (one rounding less: inside).  Every term is affine in |g| and |xhat| with
    per-channel coefficients, which is how it is evaluated (class _Aff).

ONE 16-BIT STORE of y and dx, as ref64.epilogue: U16 * (|V| + e) with U16 = 2^-8 (bf16), 2^-11 (fp16), + 2^-25 absolute for fp16
subnormals.  Every bound carries 2^-133 absolute for results in the subnormal range of f32 / bf16 (none is expected).

ASSUMPTIONS, all of them: round-to-nearest f32 operations without flushing of normal results; 2 <= n < 2^24 for the dx bound
(n = 1 is covered: M holds the same terms); the mean and invstd handed to the backward are the forward's (within Bm, Bi); the
division 1.0f / n within 2.5 ulp.  No assumption on the order of any sum, the number of partials or the grid.

WHAT THE BOUND DOES NOT PROMISE TO SEE.  Rows lost from a sum (the last row of each workgroup's range: 256 of n) move the mean by
256 / n of a term.  With the inputs of the tests that is 10^3 to 10^6 bounds of save_mean, dbeta and of the elements of y and dx that
lie near zero (tests/test_ref64_bn.py plants it), but it depends on the data: centred data whose lost rows happen to cancel would
pass.  The GPU cases therefore ALSO run integer inputs (exact_sums): every sum is exact in f64 in any order, the outputs are f32
roundings of exact numbers, and the comparison is bit for bit."""
import numpy as np
import torch

from ref64 import FP16_SUBNORMAL, U16

U32 = 2.0 ** -24
V64 = 2.0 ** -53
TINY = 2.0 ** -133
INV_N = 7 * U32               # the f32 reciprocal of n (6 u) and the product it enters (u)
UP = U32 + 2.0 ** -48         # an f32 addition plus this module's own f64 operations
F64 = torch.float64


def _t(a, n=None):
    """float64 on the CPU (the first n rows only: sliced before it is converted)"""
    if not isinstance(a, torch.Tensor):
        a = torch.as_tensor(np.asarray(a))
    a = a.detach()
    return (a if n is None else a[:n]).to("cpu").to(F64)


def f32(v):
    return float(np.float32(v))


def _store16(V, e, out_dtype):
    if out_dtype != torch.float32:
        e = e + U16[out_dtype] * (V.abs() + e)
        if out_dtype == torch.float16:
            e = e + FP16_SUBNORMAL
    return e + TINY


class Stats:
    """per channel (float64, shape (C,)): mean, var (biased), invstd and their bounds; n"""


def stats(x, n, eps):
    """the batch statistics of the first n rows of x (cap, C) and the bounds of the stored f32 mean / invstd"""
    x = _t(x, n)
    C = x.shape[1]
    s = Stats()
    s.n, s.eps = n, f32(eps)
    if n == 0:      # the kernel documents mean = 0, var = 0
        s.mean, s.var, A1 = torch.zeros(C, dtype=F64), torch.zeros(C, dtype=F64), torch.zeros(C, dtype=F64)
    else:
        s.mean = x.sum(0) / n
        A1 = x.abs().sum(0) / n
        xc = x - s.mean
        s.var = (xc * xc).sum(0) / n
        del xc
    m2 = s.mean * s.mean
    ex2 = s.var + m2
    s.E_mean = n * 2 * V64 * A1 + 2 * V64 * s.mean.abs()
    s.B_mean = s.E_mean + U32 * (s.mean.abs() + s.E_mean) + TINY
    s.E_var = n * 2 * V64 * (ex2 + 2 * s.mean.abs() * A1) + 8 * V64 * (ex2 + m2)
    s.invstd = 1.0 / torch.sqrt(s.var + s.eps)
    lo = (s.var - s.E_var).clamp_min(0.0) + s.eps
    s.E_invstd = 0.5 * s.E_var * lo ** -1.5 + 8 * V64 * s.invstd
    s.B_invstd = s.E_invstd + U32 * (s.invstd + s.E_invstd) + TINY
    return s


def _dxh(s):
    """error of the f32 xhat = (x - mean_f) * invstd_f as alpha + beta * |xhat| (per channel)"""
    k = (1 + U32) ** 2
    isb = s.invstd + s.B_invstd
    return k * s.B_mean * isb, k * (s.B_invstd + 2 * U32 * isb) / s.invstd


def forward(x, n, gamma, beta, eps, residual=None, relu=True, running_mean=None, running_var=None, momentum=0.1,
            out_dtype=torch.float32, st=None):
    """-> dict name -> (value, bound), float64: mean, invstd (C,), y (n, C) and, with running statistics, running_mean and
    running_var (C,).  `st`: the Stats of (x, n, eps) when the caller has them already."""
    s = st if st is not None else stats(x, n, eps)
    assert s.n == n and s.eps == f32(eps)
    g, b = _t(gamma), _t(beta)
    out = {"mean": (s.mean, s.B_mean), "invstd": (s.invstd, s.B_invstd)}
    if running_mean is not None and n > 0:
        mom = f32(momentum)
        rm, rv = _t(running_mean), _t(running_var)
        unb = s.var * (n / (n - 1.0)) if n > 1 else s.var
        for name, old, new, e_new in (("running_mean", rm, s.mean, s.E_mean), ("running_var", rv, unb, s.E_var * (n / (n - 1.0) if n > 1 else 1.0))):
            val = (1.0 - mom) * old + mom * new
            e = mom * e_new + 8 * V64 * (((1.0 - mom) * old).abs() + (mom * new).abs() + mom * e_new)
            out[name] = (val, e + U32 * (val.abs() + e) + TINY)
    elif running_mean is not None:      # n == 0: untouched
        out["running_mean"] = (_t(running_mean), torch.zeros_like(s.mean))
        out["running_var"] = (_t(running_var), torch.zeros_like(s.mean))
    xh = _t(x, n) - s.mean
    xh *= s.invstd
    al, be = _dxh(s)
    D = xh.abs()
    D *= (be * g.abs() * (1 + U32) + U32 * g.abs())
    D += al * g.abs() * (1 + U32)
    V = xh
    V *= g
    V += b
    D *= (1 + UP)
    D += UP * V.abs()
    if residual is not None:
        V += _t(residual, n)
        D *= (1 + UP)
        D += UP * V.abs()
    if relu:
        V.clamp_min_(0.0)
    out["y"] = (V, _store16(V, D, out_dtype))
    return out


class _Aff:
    """c0 + cg * |g| + cx * |xhat| with per-channel coefficients (float64 (C,))"""

    def __init__(self, c0, cg, cx):
        self.c = (c0, cg, cx)

    def __add__(self, o):
        return _Aff(*[a + b for a, b in zip(self.c, o.c)])

    def __mul__(self, k):
        return _Aff(*[a * k for a in self.c])

    __rmul__ = __mul__


def backward(dy, x, y_stored, n, gamma, eps, relu=True, out_dtype=torch.float32, st=None):
    """-> dict name -> (value, bound), float64: dbeta, dgamma (C,), dx, dres (n, C).  The mask is y_stored > 0."""
    s = st if st is not None else stats(x, n, eps)
    assert s.n == n and s.eps == f32(eps)
    gam = _t(gamma)
    g = _t(dy, n)
    if relu:
        g = g * (_t(y_stored, n) > 0)
    xh = _t(x, n) - s.mean
    xh *= s.invstd
    ag, axh = g.abs(), xh.abs()
    db = g.sum(0)
    dg = (g * xh).sum(0)
    Sg = ag.sum(0)
    Sgx = (ag * axh).sum(0)
    zero = torch.zeros_like(db)
    al, be = _dxh(s)
    E = n * 2 * V64 * Sg
    B_db = E + U32 * (db.abs() + E) + TINY
    first = al * Sg + be * Sgx
    E = first + (n + 8) * 2 * V64 * (Sgx + first)
    B_dg = E + U32 * (dg.abs() + E) + TINY
    out = {"dbeta": (db, B_db), "dgamma": (dg, B_dg), "dres": (g, torch.zeros(1, dtype=F64))}
    if n == 0:
        out["dx"] = (g, torch.zeros(1, dtype=F64))
        return out
    inv = 1.0 / n
    adb, adg = db.abs(), dg.abs()
    Eq1 = _Aff(B_db * inv * (1 + INV_N) + INV_N * adb * inv, zero, zero)
    Es1 = Eq1 + U32 * (_Aff(adb * inv, zero + 1.0, zero) + Eq1)
    Eq2 = _Aff(al, zero, be) * ((adg + B_dg) * (1 + U32)) + _Aff(zero, zero, B_dg + U32 * (adg + B_dg))
    Eq3 = Eq2 * (inv * (1 + INV_N)) + _Aff(zero, zero, INV_N * adg * inv)
    M = _Aff(adb * inv, zero + 1.0, adg * inv)
    Es2 = Es1 + Eq3 + U32 * (M + Es1 + Eq3)
    gi = gam.abs() * s.invstd
    Ep = gam.abs() * (s.B_invstd + U32 * (s.invstd + s.B_invstd))
    Edx = (M + Es2) * Ep + Es2 * gi + (M + Es2) * (U32 * (gi + Ep)) + M * (2.0 ** -48 * gi)
    c0, cg, cx = Edx.c
    e = ag
    e *= cg
    axh *= cx
    e += axh
    e += c0
    del axh
    # dx = gamma * invstd * (g - dbeta / n - xhat * dgamma / n)
    xh *= dg * inv
    dx = g - xh
    dx -= db * inv
    dx *= gam * s.invstd
    out["dx"] = (dx, _store16(dx, e, out_dtype))
    return out


# ------------------------------------------------------------------------------------------------ exact cases (bound zero)
def exact_sums(x, dy, y, n, relu):
    """integer inputs: sum x and sum g per channel as exact integers (int64), g = dy * [y > 0]"""
    xi = torch.as_tensor(np.asarray(x))[:n].to(torch.int64)
    g = torch.as_tensor(np.asarray(dy))[:n].to(torch.int64)
    if relu:
        g = g * (torch.as_tensor(np.asarray(y))[:n] > 0)
    return xi.sum(0), g.sum(0), (g * xi).sum(0)


def f32_of_ratio(num, den):
    """float32(float64(num) / den) for exact integers num (|num| < 2^53): what a kernel that sums exactly in f64 must store"""
    return (num.to(F64) / float(den)).to(torch.float32)
