"""A plain float64 reference of BatchNorm2d in TRAINING mode + ReLU on rows that stand for a dense map (csrc/bev_bn.hip:
fnp_bev_bn_train_forward / fnp_bev_bn_train_backward), written from the formulas of that file's header, with an error bound per
output that is DERIVED and not tuned, an independent dense route through torch's float64 conv2d / batch_norm / autograd, an f32
evaluation with plantable defects, and the checks the GPU tests apply — kept here so that tests/test_ref_bev_train.py can plant
defects and see them rejected without a device.  A helper like tests/ref64_bn.py (on which it builds), not a fixture; nothing of
the device library is imported.

THE OPERATION.  x (n, C): the values of the n cells that have a row; the other N - n of the N = B * H * W cells hold 0.
    forward :  mean = sum_r x / N,  var = sum_r x^2 / N - mean^2 = (sum_r (x - mean)^2 + (N - n) mean^2) / N,
               invstd = 1 / sqrt(var + eps),  running statistics with var * N / (N - 1),
               y_r = relu((x_r - mean) * invstd * gamma + beta),  fill = relu((0 - mean) * invstd * gamma + beta)
    backward:  g_r = G_r * [y_r stored > 0],  gate = [fill stored > 0],  Dbg = sum of G over the cells without a row (= T - R),
               dbeta = sum_r g + gate * Dbg,  dgamma = sum_r g * xhat_r + gate * xhat_bg * Dbg,  xhat_bg = (0 - mean) * invstd,
               dx_r = gamma * invstd * (g_r - dbeta / N - xhat_r * dgamma / N)
Both masks are taken from what the kernel STORED (the y it wrote at the row cells, the fill it wrote), as tests/ref64_bn.py
defines its mask: that is the definition of the operation, so there is no allowance for an element "on the other side".

THE BOUNDS are those of tests/ref64_bn.py with N in place of n — the kernel adds n <= N terms, so every `n * 2^-52 * sum |term|`
of that derivation holds with N, and 1.0f / N takes the place of 1.0f / n — plus the terms of the background:
  * var: the zeros add (N - n) mean^2 / N to it; in the kernel's form E[x^2] - mean^2 they are not terms at all.  stats() below
    evaluates ref64_bn's E_var with Ex2 = var + mean^2 and A1 = sum |x| / N: unchanged in form.
  * fill: a row with x = 0 through the forward apply: ref64_bn.forward's bound of such a row (d = |0 - mean|), f32.
  * T - R.  The kernel forms T = sum over ALL cells of G and R = sum over the row cells in f64 and subtracts; this module adds the
    cells without a row directly.  Each f64 sum of at most N terms errs by N * 2^-53 * sum |term| on each side; the difference
    inherits both ABSOLUTE errors however small it is (the cancellation):
        E_D = N * 2^-52 * (sum_all |G| + sum_rows |G|) + 2^-52 * |Dbg|
  * dbeta:   E = N * 2^-52 * sum_r |g| + gate * E_D + 2^-52 * |dbeta|,                         B = E + u (|dbeta| + E)
  * dgamma:  the rows' part as ref64_bn (with N); the background's: xhat_bg is an f32 value with the error of any f32 xhat,
    Dxh(0) = alpha + beta_x |xhat_bg| (ref64_bn._dxh), multiplied in f64 by a difference that carries E_D:
        E_bg = gate * (Dxh(0) * (|Dbg| + E_D) + |xhat_bg| * E_D),   E = E_rows + E_bg + 2^-51 * (|xhat_bg Dbg| + |dgamma|)
  * the gate itself adds nothing: it is read from the stored fill, like the rows' mask from the stored y.
  * dx: ref64_bn's nine roundings with N, fed the dbeta / dgamma bounds above.
ASSUMPTIONS: those of ref64_bn (round-to-nearest f32 without flushing, N < 2^24, 1.0f / N within 2.5 ulp)."""
import numpy as np
import torch

import ref64 as R
import ref64_bn as RBN
from ref64_bn import F64, INV_N, TINY, U32, V64, _Aff, _dxh, _store16, _t, f32

EPS, MOMENTUM = 1e-3, 0.01          # BaseBEVBackbone's BatchNorm2d


# ------------------------------------------------------------------------------------------------ the operator in float64
def stats(x, n, N, eps):
    """ref64_bn.Stats of the N cells: the first n rows of x and N - n zeros"""
    x = _t(x, n)
    s = RBN.Stats()
    s.n, s.eps, s.rows = N, f32(eps), n
    s.mean = x.sum(0) / N
    A1 = x.abs().sum(0) / N
    xc = x - s.mean
    s.var = ((xc * xc).sum(0) + (N - n) * s.mean * s.mean) / N
    m2 = s.mean * s.mean
    ex2 = s.var + m2
    s.E_mean = N * 2 * V64 * A1 + 2 * V64 * s.mean.abs()
    s.B_mean = s.E_mean + U32 * (s.mean.abs() + s.E_mean) + TINY
    s.E_var = N * 2 * V64 * (ex2 + 2 * s.mean.abs() * A1) + 8 * V64 * (ex2 + m2)
    s.invstd = 1.0 / torch.sqrt(s.var + s.eps)
    lo = (s.var - s.E_var).clamp_min(0.0) + s.eps
    s.E_invstd = 0.5 * s.E_var * lo ** -1.5 + 8 * V64 * s.invstd
    s.B_invstd = s.E_invstd + U32 * (s.invstd + s.E_invstd) + TINY
    return s


def forward(x, n, N, gamma, beta, eps=EPS, running_mean=None, running_var=None, momentum=MOMENTUM, out_dtype=torch.float32, st=None):
    """-> dict name -> (value, bound), float64: mean, invstd, fill (C,), y (n, C) at the row cells, running_mean, running_var.
    fill's bound is that of an f32 value (the kernel stores it in f32); y's includes the store in out_dtype."""
    s = st if st is not None else stats(x, n, N, eps)
    C = s.mean.shape[0]
    assert n <= N
    # ref64_bn.forward with the Stats of the N cells: it slices x[:N] (the n rows there are) and takes N for the running variance
    out = RBN.forward(_t(x, n), N, gamma, beta, eps, relu=True, running_mean=running_mean, running_var=running_var, momentum=momentum,
                      out_dtype=out_dtype, st=s)
    # ... and once more on a single cell with x = 0
    V, e = RBN.forward(torch.zeros((1, C), dtype=F64), N, gamma, beta, eps, relu=True, out_dtype=torch.float32, st=s)["y"]
    out["fill"] = (V[0], e[0])
    return out


def backward(G_rows, G_sum_all, G_abs_all, x, y_rows_stored, fill_stored, n, N, gamma, eps=EPS, out_dtype=torch.float32, st=None):
    """G_rows (n, C): the gradient map at the row cells; G_sum_all, G_abs_all (C,): sum of G and of |G| over ALL cells in float64.
    -> dict name -> (value, bound): dbeta, dgamma (C,), dx (n, C)."""
    s = st if st is not None else stats(x, n, N, eps)
    gam = _t(gamma)
    Gr = _t(G_rows, n)
    g = Gr * (_t(y_rows_stored, n) > 0)
    gate = (_t(fill_stored) > 0).to(F64)
    xh = _t(x, n) - s.mean
    xh *= s.invstd
    ag, axh = g.abs(), xh.abs()
    SGr = Gr.abs().sum(0)
    Dbg = _t(G_sum_all) - Gr.sum(0)                                           # (this module's own cancellation: 2^-52 (SGall + SGr), inside E_D)
    SGall = _t(G_abs_all)
    E_D = N * 2 * V64 * (SGall + SGr) + 2 * V64 * Dbg.abs()
    xhbg = (0.0 - s.mean) * s.invstd
    al, be = _dxh(s)
    Sg, Sgx = ag.sum(0), (ag * axh).sum(0)
    db = g.sum(0) + gate * Dbg
    dg = (g * xh).sum(0) + gate * xhbg * Dbg
    E = N * 2 * V64 * Sg + gate * E_D + 2 * V64 * db.abs()
    B_db = E + U32 * (db.abs() + E) + TINY
    first = al * Sg + be * Sgx
    E_rows = first + (N + 8) * 2 * V64 * (Sgx + first)
    dxh0 = al + be * xhbg.abs()
    E_bg = gate * (dxh0 * (Dbg.abs() + E_D) + xhbg.abs() * E_D)
    E = E_rows + E_bg + 4 * V64 * ((xhbg * Dbg).abs() + dg.abs())
    B_dg = E + U32 * (dg.abs() + E) + TINY
    out = {"dbeta": (db, B_db), "dgamma": (dg, B_dg)}
    zero = torch.zeros_like(db)
    inv = 1.0 / N
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
    e = ag * cg + axh * cx + c0
    dx = (g - db * inv - xh * (dg * inv)) * (gam * s.invstd)
    out["dx"] = (dx, _store16(dx, e, out_dtype))
    return out


# ------------------------------------------------------------------------------------------------ the dense route (independent)
def dense_route(idx, feats, B, shape, w2d, gamma, beta, running_mean, running_var, G, eps=EPS, momentum=MOMENTUM):
    """pad -> conv2d -> F.batch_norm(training=True) -> relu in torch float64 on the CPU, and autograd.grad for the gradient map G
    (B, Cout, H, W): -> dict y (B, Cout, H, W), running_mean, running_var, dfeats (n, C), dW (Cout, C * D, 3, 3), dgamma, dbeta.
    Shares no code with the row form; small maps only."""
    D, H, W = shape
    idx = np.asarray(idx).astype(np.int64)
    f = lambda a: torch.as_tensor(np.asarray(a, np.float64) if not isinstance(a, torch.Tensor) else a.detach().cpu().double().numpy())
    x = f(feats).requires_grad_(True)
    C = x.shape[1]
    m = torch.zeros((B, C, D, H, W), dtype=F64)
    m[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]] = x
    m = m.view(B, C * D, H, W)
    w, ga, be = f(w2d).requires_grad_(True), f(gamma).requires_grad_(True), f(beta).requires_grad_(True)
    rm, rv = f(running_mean).clone(), f(running_var).clone()
    z = torch.nn.functional.conv2d(torch.nn.functional.pad(m, (1, 1, 1, 1)), w)
    y = torch.relu(torch.nn.functional.batch_norm(z, rm, rv, ga, be, True, float(np.float32(momentum)), float(np.float32(eps))))
    dx, dw, dga, dbe = torch.autograd.grad(y, (x, w, ga, be), f(G))
    return dict(y=y.detach(), z=z.detach(), running_mean=rm, running_var=rv, dfeats=dx, dW=dw, dgamma=dga, dbeta=dbe)


def weight_to_2d(dw_packed, D):
    """(K = D * 9, Cout, C) -> (Cout, C * D, 3, 3): the inverse of ref_bev.weight3d (2D channel c * D + z)"""
    dw = np.asarray(dw_packed)
    K, Cout, C = dw.shape
    out = np.empty((Cout, C * D, 3, 3), dw.dtype)
    for z in range(D):
        for ky in range(3):
            for kx in range(3):
                out[:, z::D, ky, kx] = dw[(z * 3 + ky) * 3 + kx]
    return out


# ------------------------------------------------------------------------------------------------ inputs of the operator tests
def draw_operator(name_seed, n, C, td):
    """rows x (n, C) with a per-channel offset of both signs (so that mean != 0 and fill has both gates), row 0 all zeros (a row
    cell whose value is the background's: its y must equal fill in its bits), gamma in U(0.5, 1.5), beta of alternating sign and
    magnitude 0.3 .. 0.6, running statistics, all f32 (x rounded to td)"""
    rng = np.random.default_rng(4000 + name_seed)
    x = (rng.standard_normal((n, C)) + rng.uniform(-0.5, 0.5, C)).astype(np.float32)
    x[0] = 0.0
    if td != torch.float32:
        x = R.round16(x, td)
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    beta = (rng.uniform(0.3, 0.6, C) * np.where(np.arange(C) % 2 == 0, 1.0, -1.0)).astype(np.float32)
    rm = (rng.standard_normal(C) * 0.2).astype(np.float32)
    rv = rng.uniform(0.5, 1.5, C).astype(np.float32)
    return x, gamma, beta, rm, rv


def draw_gradient(name_seed, B, C, H, W, td):
    G = np.random.default_rng(5000 + name_seed).standard_normal((B, C, H, W)).astype(np.float32)
    return G if td == torch.float32 else R.round16(G, td)


def gates_exercised(fill64):
    """at least a quarter of the channels with fill > 0 and a quarter with fill = 0 (asserted on the REFERENCE before any device
    result is looked at)"""
    f = np.asarray(fill64)
    return (f > 0).sum() * 4 >= f.shape[0] and (f == 0).sum() * 4 >= f.shape[0]


# ------------------------------------------------------------------------------------------------ f32 evaluation with defects
DEFECTS = ("stats over rows", "unbiased n", "unbiased left out", "background left out", "background ungated", "fill without relu",
           "xhat_bg zero")


def evaluate32(x, sites, n, B, H, W, gamma, beta, rm, rv, G, td, defect=None, eps=EPS, momentum=MOMENTUM):
    """the operator in numpy: sums in float64 (as the kernel), everything else in f32 with the kernel's operation order; `defect`
    plants one of DEFECTS.  -> dict of arrays named as the kernel's outputs (y: the dense map in td's rounding, as f32)"""
    assert defect is None or defect in DEFECTS
    f = np.float32
    x = np.asarray(x, f)[:n]
    C = x.shape[1]
    N = B * H * W
    Ns = n if defect == "stats over rows" else N
    m64 = x.astype(np.float64).sum(0) / Ns
    var64 = np.maximum((x.astype(np.float64) ** 2).sum(0) / Ns - m64 * m64, 0.0)
    mean, invstd = m64.astype(f), (1.0 / np.sqrt(var64 + np.float64(f(eps)))).astype(f)
    unb = {"unbiased n": n / (n - 1.0), "unbiased left out": 1.0}.get(defect, Ns / (Ns - 1.0))
    mom = np.float64(f(momentum))
    out = dict(save_mean=mean, save_invstd=invstd,
               running_mean=((1 - mom) * np.asarray(rm, np.float64) + mom * m64).astype(f),
               running_var=((1 - mom) * np.asarray(rv, np.float64) + mom * var64 * unb).astype(f))
    gamma, beta = np.asarray(gamma, f), np.asarray(beta, f)
    rnd = (lambda a: a) if td == torch.float32 else (lambda a: torch.from_numpy(np.ascontiguousarray(a, f)).to(td).float().numpy())
    apply = lambda v: (v - mean) * invstd * gamma + beta
    fill = apply(np.zeros(C, f))
    if defect != "fill without relu":
        fill = np.maximum(fill, f(0))
    yr = rnd(np.maximum(apply(x), f(0)))
    y = np.empty((B, C, H, W), f)
    y[:] = rnd(fill).reshape(1, C, 1, 1)
    s = np.asarray(sites)[:n].astype(np.int64)
    y[s[:, 0], :, s[:, 2], s[:, 3]] = yr
    out.update(fill=fill.astype(f), y=y)
    G = np.asarray(G, f)
    Gr = G[s[:, 0], :, s[:, 2], s[:, 3]]
    g = np.where(yr > 0, Gr, f(0))
    xh = (x - mean) * invstd
    Dbg = G.astype(np.float64).sum((0, 2, 3)) - Gr.astype(np.float64).sum(0)
    gate = np.ones(C) if defect == "background ungated" else (fill > 0).astype(np.float64)
    if defect == "background left out":
        gate = np.zeros(C)
    xhbg = np.zeros(C, f) if defect == "xhat_bg zero" else (f(0) - mean) * invstd
    db = (g.astype(np.float64).sum(0) + gate * Dbg).astype(f)
    dg = ((g.astype(np.float64) * xh.astype(np.float64)).sum(0) + gate * xhbg.astype(np.float64) * Dbg).astype(f)
    inv_n = f(1.0) / f(Ns)
    dx = gamma * invstd * (g - db * inv_n - xh * dg * inv_n)
    out.update(dbeta=db, dgamma=dg, dx=rnd(dx.astype(f)))
    return out


# ------------------------------------------------------------------------------------------------ the checks
def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def reference(x, sites, n, B, H, W, gamma, beta, rm, rv, td, eps=EPS, momentum=MOMENTUM):
    """the forward reference of a case (float64 values with bounds) and its Stats"""
    st = stats(x, n, B * H * W, eps)
    return st, forward(x, n, B * H * W, gamma, beta, eps, rm, rv, momentum, out_dtype=td, st=st)


def check_forward(got, fwd, sites, n, td):
    """got: dict of f32 numpy arrays save_mean, save_invstd, fill, running_mean, running_var, y (B, C, H, W) (16-bit maps widened
    to f32).  -> list of findings (empty: right) and dict of worst err / bound"""
    fail, worst = [], {}
    for name, key in (("save_mean", "mean"), ("save_invstd", "invstd"), ("fill", "fill"), ("running_mean", "running_mean"),
                      ("running_var", "running_var")):
        V, e = fwd[key]
        w, rep = R.check(np.asarray(got[name])[None], V[None], e[None])
        worst[name] = w
        if rep is not None:
            fail.append(f"{name}: {rep}")
    y = np.asarray(got["y"])
    B, C, H, W = y.shape
    s = np.asarray(sites)[:n].astype(np.int64)
    V, e = fwd["y"]
    w, rep = R.check(y[s[:, 0], :, s[:, 2], s[:, 3]], V, e)
    worst["y"] = w
    if rep is not None:
        fail.append("y at the row cells: " + rep)
    site = np.zeros((B, H, W), bool)
    site[s[:, 0], s[:, 2], s[:, 3]] = True
    assert int(site.sum()) == n
    fill = np.asarray(got["fill"], np.float32)
    bg = fill if td == torch.float32 else torch.from_numpy(fill).to(td).float().numpy()
    bad = (_bits(y) != _bits(bg).reshape(1, C, 1, 1)).any(1) & ~site
    if bad.any():
        cells = np.argwhere(bad)
        fail.append(f"background: {cells.shape[0]} of {int((~site).sum())} cells without a row differ from fill in their bits, first (b, y, x) {cells[:6].tolist()}")
    return fail, worst


def check_backward(got, x, G, y_map, fill, sites, n, B, H, W, gamma, td, st, eps=EPS):
    """got: dict dbeta, dgamma (C,), dx (cap, C) f32 numpy.  The masks come from y_map / fill, the maps the device stored."""
    s = np.asarray(sites)[:n].astype(np.int64)
    G = np.asarray(G, np.float32)
    G64 = torch.from_numpy(G).to(F64)
    ref = backward(G[s[:, 0], :, s[:, 2], s[:, 3]], G64.sum((0, 2, 3)), G64.abs().sum((0, 2, 3)), x, np.asarray(y_map)[s[:, 0], :, s[:, 2], s[:, 3]],
                   fill, n, B * H * W, gamma, eps, out_dtype=td, st=st)
    fail, worst = [], {}
    for name in ("dbeta", "dgamma"):
        V, e = ref[name]
        w, rep = R.check(np.asarray(got[name])[None], V[None], e[None])
        worst[name] = w
        if rep is not None:
            fail.append(f"{name}: {rep}")
    V, e = ref["dx"]
    dx = np.asarray(got["dx"])
    w, rep = R.check(dx[:n], V, e)
    worst["dx"] = w
    if rep is not None:
        fail.append("dx: " + rep)
    if (_bits(dx[n:]) != 0).any():
        fail.append(f"dx: {int((_bits(dx[n:]) != 0).any(1).sum())} rows behind n are not exactly 0")
    return fail, worst
