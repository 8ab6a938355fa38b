"""The adam_onecycle optimizer step of include/fnp.h (fnp_adam_onecycle_step) restated in f64 numpy, a roundoff bound for an
f32 evaluation of it, four wrong variants, and the golden record of the reference's run (tests/golden/adam_onecycle_golden.npz,
written by tests/golden/make_adam_onecycle_golden.py).

A state is a dict: p, m, v (lists of 1-D f64 arrays, one per tensor), t (int array, one per tensor), scale (float or None:
no scaler), tracker (int).  A step's inputs: grads (list of arrays as they come, scaled; None: no gradient) and hp, a dict of
lr, beta1, beta2, eps, wd, max_norm, growth_factor, backoff_factor, growth_interval.

THE BOUND.  u = 2^-24 (f32 unit roundoff); every f32 operation (multiply, add, divide, square root: IEEE, no fused
multiply-add) and every rounding of an f64 scalar to f32 costs a relative u.  The inputs (p, m, v, g) are f32 values that the
two evaluations share; the scale is a power of two or not, inv is f32 in the contract itself.  Per element, first order in u,
with d(x) the bound on |x_f32 - x_f64|:
  g^ = g * inv                       1 rounding                                     d(g^) = u |g^|
  N: from the rounded g^ (relative u on every term, so at most u on N; the f64 sum itself adds nothing at this level)
  c = (float)min(1, max_norm/(N+1e-6))   u from N, u from the rounding                 d(c) = 2u c
  g' = g^ * c                        u + 2u + 1 rounding                               d(g') = 4u |g'|
  e = (g' - m) * (float)(1 - beta1)  the difference CANCELS: its error is absolute,
                                     roundings of g' - m: d(g') + u |g' - m| <= d(g') + u (|g'| + |m|);
                                     then u for the scalar and u for the product       d(e) = (1-beta1) (d(g') + 3u (|g'| + |m|))
  m' = m + e                         1 rounding; what m_in carries passes through the exact map m' = beta1 m + (1-beta1) g'
                                                                                       d(m') = beta1 d(m_in) + d(e) + u |m'|
  v' = (float)beta2 * v + ((float)(1-beta2) * g') * g'
                                     first term: u scalar + u product; second: u scalar, 2 * 4u from g', 2 products
                                                                                       d(v') = beta2 d(v_in) + 2u beta2 v + 11u (1-beta2) g'^2 + u v'
  s = sqrt(v')                       |sqrt(v' +- d(v')) - sqrt(v')| + 1 rounding       d(s) = sqrt(v') - sqrt(max(v' - d(v'), 0)) + u s
  q = s / (float)sqrt(1 - beta2^t)   u scalar + u quotient                             d(q) = d(s) / bc2 + 2u q
  den = q + (float)eps               u on eps, 1 rounding                              d(den) = d(q) + u eps + u den
  r = m' / den                       1 rounding                                        d(r) = (d(m') + |r| d(den)) / (den - d(den)) + u |r|
  w = (float)(lr/(1-beta1^t)) * r    u scalar + u product                              d(w) = ss d(r) + 2u |w|
  p1 = p * (float)(1 - wd lr)        u scalar + u product                              d(p1) = decay d(p_in) + 2u |p1|
  p' = p1 - w                        1 rounding                                        d(p') = d(p1) + d(w) + u |p'|
A tensor without a gradient: p' = p1 alone, m and v untouched.  The whole is multiplied by 1 + 64u for the second-order
terms (the longest chain above has fewer than 32 roundings).  Over k steps the d(.)_in of a step are the d(.)' of the step
before (bound(..., carry)); one step from exact inputs has them 0.  Nothing here is fitted to what any implementation gives."""
import os

import numpy as np

U = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adam_onecycle_golden.npz")
VARIANTS = ("decay_after_adam", "bias_from_t_minus_1", "beta1_of_first_step", "clip_without_1e-6")


def unscale_norm(state, grads):
    """inv, the unscaled gradients, N and found_inf (steps 1 and 2 of the contract)"""
    inv = 1.0 if state["scale"] is None else float(np.float32(1.0 / np.float64(np.float32(state["scale"]))))
    with np.errstate(invalid="ignore", over="ignore"):
        gh = [None if g is None else np.asarray(g, np.float64) * inv for g in grads]
        found = any(g is not None and not np.isfinite(g).all() for g in gh)
        total = sum(float((g * g).sum()) for g in gh if g is not None)
        return inv, gh, float(np.sqrt(total)), found


def step(state, grads, hp, variant=None, beta1_first=None):
    """one step in f64 -> (new state, N, found_inf); `variant`: one of VARIANTS, a wrong rule in place of the contract's"""
    assert variant is None or variant in VARIANTS
    lr, b1, b2, eps, wd = hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"]
    _, gh, norm, found = unscale_norm(state, grads)
    new = {"p": [x.copy() for x in state["p"]], "m": [x.copy() for x in state["m"]], "v": [x.copy() for x in state["v"]],
           "t": np.array(state["t"]).copy(), "scale": state["scale"], "tracker": state["tracker"]}
    if found:
        if state["scale"] is not None:
            new["scale"], new["tracker"] = state["scale"] * hp["backoff_factor"], 0
        return new, norm, True
    with np.errstate(divide="ignore", invalid="ignore"):
        floor = norm + (0.0 if variant == "clip_without_1e-6" else 1e-6)
        clip = min(1.0, hp["max_norm"] / floor) if floor > 0 else 1.0
        decay = 1.0 - wd * lr
        for i, g in enumerate(gh):
            if variant != "decay_after_adam":
                new["p"][i] *= decay
            if g is not None:
                new["t"][i] += 1
                t = int(new["t"][i]) - (1 if variant == "bias_from_t_minus_1" else 0)
                gp = g * clip
                new["m"][i] = new["m"][i] + (gp - new["m"][i]) * (1.0 - b1)
                new["v"][i] = b2 * new["v"][i] + (1.0 - b2) * gp * gp
                bc1 = 1.0 - (beta1_first if variant == "beta1_of_first_step" else b1) ** t
                den = np.sqrt(new["v"][i]) / np.sqrt(1.0 - b2 ** t) + eps
                new["p"][i] = new["p"][i] - np.float64(lr) / np.float64(bc1) * (new["m"][i] / den)
            if variant == "decay_after_adam":
                new["p"][i] *= decay
    if state["scale"] is not None:
        new["tracker"] = state["tracker"] + 1
        if new["tracker"] == hp["growth_interval"]:
            grown = state["scale"] * hp["growth_factor"]
            if np.isfinite(np.float32(grown)):
                new["scale"] = grown
            new["tracker"] = 0
    return new, norm, False


def bound(state, grads, hp, carry=None):
    """per-element bounds (dp, dm, dv: lists of arrays) on |f32 evaluation - f64 evaluation| of one step from `state`; carry:
    the (dp, dm, dv) the state itself already carries (None: the two evaluations start from the same values)"""
    lr, b1, b2, eps, wd = hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"]
    zeros = [np.zeros_like(x) for x in state["p"]]
    dp_in, dm_in, dv_in = carry if carry is not None else (zeros, zeros, zeros)
    _, gh, norm, found = unscale_norm(state, grads)
    if found:
        return [x.copy() for x in dp_in], [x.copy() for x in dm_in], [x.copy() for x in dv_in]
    new, _, _ = step(state, grads, hp)
    clip = min(1.0, hp["max_norm"] / (norm + 1e-6))
    decay, slack = abs(1.0 - wd * lr), 1.0 + 64 * U
    dp, dm, dv = [], [], []
    for i, g in enumerate(gh):
        p_in, m_in, v_in = state["p"][i], state["m"][i], state["v"][i]
        p1 = p_in * (1.0 - wd * lr)
        d_p1 = decay * dp_in[i] + 2 * U * np.abs(p1)
        if g is None:
            dp.append(d_p1 * slack); dm.append(dm_in[i].copy()); dv.append(dv_in[i].copy())
            continue
        t = int(new["t"][i])
        gp = np.abs(g * clip)
        m_abs = np.abs(m_in) + dm_in[i]
        d_e = (1.0 - b1) * (4 * U * gp + 3 * U * (gp + m_abs))
        m1, v1 = new["m"][i], new["v"][i]
        d_m = b1 * dm_in[i] + d_e + U * (np.abs(m1) + dm_in[i] + d_e)
        d_v = b2 * dv_in[i] + 2 * U * b2 * (v_in + dv_in[i]) + 11 * U * (1.0 - b2) * gp * gp + U * (v1 + dv_in[i])
        s = np.sqrt(v1)
        d_s = np.maximum(s - np.sqrt(np.maximum(v1 - d_v, 0.0)), np.sqrt(v1 + d_v) - s) + U * np.sqrt(v1 + d_v)
        bc2 = np.sqrt(1.0 - b2 ** t)
        q = s / bc2
        d_q = d_s / bc2 + 2 * U * (q + d_s / bc2)
        den = q + eps
        d_den = d_q + U * eps + U * (den + d_q)
        r = np.abs(m1) / den
        d_r = (d_m + r * d_den) / (den - d_den) + U * (r + (d_m + r * d_den) / (den - d_den))
        ss = lr / (1.0 - b1 ** t)
        w = ss * r
        d_w = ss * d_r + 2 * U * (w + ss * d_r)
        d_p = d_p1 + d_w + U * (np.abs(new["p"][i]) + d_p1 + d_w)
        dp.append(d_p * slack); dm.append(d_m * slack); dv.append(d_v * slack)
    return dp, dm, dv


# ------------------------------------------------------------------------------------------------ the golden record
def split(flat, sizes):
    return [np.array(x, np.float64) for x in np.split(np.asarray(flat), np.cumsum(sizes)[:-1])]


class Golden:
    """the reference's recorded run: K = 13 records (12 iterations of the schedule, then the small-clip step)"""

    def __init__(self, path=GOLDEN):
        z = np.load(path)
        self.z = {k: z[k] for k in z.files}
        self.sizes = [int(s) for s in self.z["sizes"]]
        self.group_sizes = [int(s) for s in self.z["group_sizes"]]
        self.K = int(self.z["lr"].shape[0])
        self.steps = 12

    def hp(self, k):
        z = self.z
        return {"lr": float(z["lr"][k]), "beta1": float(z["mom"][k]), "beta2": float(z["beta2"]), "eps": float(z["eps"]),
                "wd": float(z["wd"]), "max_norm": float(z["max_norm"][k]), "growth_factor": float(z["growth_factor"]),
                "backoff_factor": float(z["backoff_factor"]), "growth_interval": int(z["growth_interval"])}

    def state_before(self, k):
        z = self.z
        if k == 0:
            p, m, v, t = z["p0"], np.zeros_like(z["p0"]), np.zeros_like(z["p0"]), np.zeros(len(self.sizes), np.int64)
        else:
            p, m, v, t = z["p"][k - 1], z["m"][k - 1], z["v"][k - 1], z["t"][k - 1]
        return {"p": split(p, self.sizes), "m": split(m, self.sizes), "v": split(v, self.sizes), "t": np.array(t, np.int64),
                "scale": float(z["scale_before"][k]), "tracker": int(z["tracker_before"][k])}

    def state_after(self, k):
        z = self.z
        return {"p": split(z["p"][k], self.sizes), "m": split(z["m"][k], self.sizes), "v": split(z["v"][k], self.sizes),
                "t": np.array(z["t"][k], np.int64), "scale": float(z["scale_after"][k]), "tracker": int(z["tracker_after"][k])}

    def grads(self, k):
        return [g if here else None for g, here in zip(split(self.z["grads"][k], self.sizes), self.z["present"][k])]


def as_f32(state):
    """the state with p, m, v rounded to f32 values (kept as f64 arrays): what an f32 implementation can start from"""
    r = lambda xs: [x.astype(np.float32).astype(np.float64) for x in xs]
    return dict(state, p=r(state["p"]), m=r(state["m"]), v=r(state["v"]))


def grads_f32(grads):
    with np.errstate(over="ignore"):
        return [None if g is None else g.astype(np.float32).astype(np.float64) for g in grads]


def tile(arrays, lengths):
    """the record's tensors laid end to end and repeated to fill tensors of `lengths` (None stays None per TARGET tensor: the
    caller decides presence)"""
    flat = np.concatenate([np.zeros(0)] + [a for a in arrays])
    total = int(sum(lengths))
    reps = -(-total // max(flat.size, 1))
    long = np.tile(flat, reps)[:total]
    return [np.array(x) for x in np.split(long, np.cumsum(lengths)[:-1])]
