"""tests/ref64_bn.py, the float64 reference of the at-scale BatchNorm tests (tests/test_gpu_bn_at_scale.py), checked on the CPU:
against torch's own F.batch_norm(training=True) and autograd in float64 (the independent check of the reference); against a
CORRECT emulation of csrc/bnorm.hip in numpy (f64 partial sums over the contiguous row ranges of the grid, in several groupings,
the finishing order, f32 apply arithmetic, one 16-bit store), which must lie inside every bound; and against PLANTED DEFECTS in
that emulation, every one of which must be rejected at the size of the GPU case named beside it, or at a size where the defect
is relatively no easier to see."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref64 as R
import ref64_bn as B
from test_gpu_bn_at_scale import EPS, MOMENTUM, draw, draw_affine, rows_per_iter, stats_grid, threshold

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
FORMS = [(True, True), (True, False), (False, True), (False, False)]       # (relu, residual)
f32 = np.float32


# ------------------------------------------------------------------------------------------------ the reference against torch
@pytest.mark.parametrize("relu,with_res", FORMS)
@pytest.mark.parametrize("C", [8, 16, 32, 64, 128, 256])
def test_reference_equals_torch_float64(C, relu, with_res):
    gen = torch.Generator().manual_seed(C)
    n, cap = 1003, 1040
    gamma, beta, rm0, rv0 = draw_affine(gen, C, "cpu")
    x = draw(gen, cap, C, torch.float32, "large" if C in (16, 128) else "unit", "cpu")
    res = torch.randn(cap, C, generator=gen) if with_res else None
    dy = torch.randn(cap, C, generator=gen)
    eps, mom = B.f32(EPS), B.f32(MOMENTUM)
    xt = x[:n].double().requires_grad_(True)
    rt = res[:n].double().requires_grad_(True) if with_res else None
    gt, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm, rv = rm0.double(), rv0.double()
    z = F.batch_norm(xt, rm, rv, gt, bt, True, mom, eps)
    z = z + rt if with_res else z
    y = torch.relu(z) if relu else z
    (y * dy[:n].double()).sum().backward()
    fw = B.forward(x, n, gamma, beta, EPS, res, relu, rm0, rv0, MOMENTUM)
    bw = B.backward(dy, x, y.detach(), n, gamma, EPS, relu)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12 * float(b.abs().max()))
    close(fw["y"][0], y.detach())
    close(fw["mean"][0], xt.detach().mean(0))
    close(fw["invstd"][0], 1.0 / torch.sqrt(xt.detach().var(0, unbiased=False) + eps))
    close(fw["running_mean"][0], rm)
    close(fw["running_var"][0], rv)
    close(bw["dx"][0], xt.grad)
    close(bw["dgamma"][0], gt.grad)
    close(bw["dbeta"][0], bt.grad)
    if with_res:
        close(bw["dres"][0], rt.grad)
    assert float(bw["dres"][1].max()) == 0.0
    for d in (fw, bw):
        for k, (v, e) in d.items():
            assert bool((e >= 0).all()) and bool(torch.isfinite(e).all()), k


def test_reference_small_frames():
    """n = 1 as the kernel documents it (running_var takes the variance itself: 0), n = 0 leaves the running statistics alone"""
    gen = torch.Generator().manual_seed(0)
    C = 16
    gamma, beta, rm0, rv0 = draw_affine(gen, C, "cpu")
    x = draw(gen, 8, C, torch.float32, "unit", "cpu")
    fw = B.forward(x, 1, gamma, beta, EPS, None, False, rm0, rv0, MOMENTUM)
    assert torch.equal(fw["mean"][0], x[0].double()) and float(fw["invstd"][0][0]) == 1.0 / np.sqrt(B.f32(EPS))
    torch.testing.assert_close(fw["running_var"][0], (1.0 - B.f32(MOMENTUM)) * rv0.double(), rtol=1e-15, atol=0)
    torch.testing.assert_close(fw["y"][0], beta.double()[None], rtol=1e-15, atol=0)
    fw = B.forward(x, 0, gamma, beta, EPS, None, False, rm0, rv0, MOMENTUM)
    assert torch.equal(fw["running_mean"][0], rm0.double()) and float(fw["running_var"][1].max()) == 0.0 and fw["y"][0].shape == (0, C)
    bw = B.backward(x, x, None, 0, gamma, EPS, False)
    assert float(bw["dbeta"][0].abs().max()) == 0.0 and float(bw["dgamma"][0].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ an emulation of the kernels
def _partials(a, b, n, G, grouping, defect):
    """part (G, C, 2): f64 sums of a and b over the grid's contiguous row ranges; within a range the rows r0 + j, r0 + j + grouping,
    ... are summed first (the threads of a workgroup), then the groups in order"""
    C = a.shape[1]
    part = np.zeros((G, C, 2))
    per = -(-n // G)
    for w in range(G):
        r0, r1 = per * w, min(n, per * w + per)
        if defect == "lost_row" and r1 > r0:
            r1 -= 1
        for j in range(grouping):
            if r0 + j < r1:
                part[w, :, 0] += a[r0 + j:r1:grouping].sum(0)
                part[w, :, 1] += b[r0 + j:r1:grouping].sum(0)
    if defect == "lost_partials":
        part[128:] = 0.0
    if defect == "lost_channel_groups" and C == 256:
        part[:, 128:] = 0.0         # (channel groups 16 - 31; the historical defect left them UNWRITTEN: zero is its mildest form)
    return part


def _finish(part):
    """thread (slice, c) adds the partials slice, slice + S, ...; the slices meet in a tree"""
    G, C, _ = part.shape
    S = 256 // min(C, 16)
    sl = [part[s::S].sum(0) if s < G else np.zeros((C, 2)) for s in range(S)]
    while len(sl) > 1:
        h = len(sl) // 2
        sl = [sl[i] + sl[i + h] for i in range(h)]
    return sl[0][:, 0], sl[0][:, 1]


def _store(a, td):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(td)


def emulate(d, n, cap, td, relu, with_res, grouping=1, defect=None, y_given=None, eps=EPS, G=256):
    """csrc/bnorm.hip on the CPU: d holds the stored inputs as f32 numpy arrays (cap rows).  -> dict of outputs like the GPU test's"""
    x, dy, gamma, beta = d["x"], d["dy"], d["gamma"], d["beta"]
    C = x.shape[1]
    eps32, mom = float(f32(eps)), float(f32(MOMENTUM))
    rows = x.shape[0] if defect == "rows_to_cap" else n         # (inputs() draws the rows up to cap only where cap - n is small)
    x64 = x[:rows].astype(np.float64)
    a, b = _finish(_partials(x64, x64 * x64, rows, G, grouping, defect))
    m = a / n if n > 0 else np.zeros(C)
    var = np.maximum(b / n - m * m, 0.0) if n > 0 else np.zeros(C)
    unb = var * (n / (n - 1.0)) if n > 1 else var
    mean_f = m.astype(f32)
    invstd_f = (1.0 / np.sqrt((unb if defect == "unbiased_invstd" else var) + eps32)).astype(f32)
    out = {"mean": torch.from_numpy(mean_f), "invstd": torch.from_numpy(invstd_f)}
    if n > 0:
        w_old, w_new = (mom, 1.0 - mom) if defect == "momentum_reversed" else (1.0 - mom, mom)
        out["running_mean"] = torch.from_numpy((w_old * d["rm"].astype(np.float64) + w_new * m).astype(f32))
        out["running_var"] = torch.from_numpy((w_old * d["rv"].astype(np.float64) + w_new * (var if defect == "biased_running_var" else unb)).astype(f32))
    else:
        out["running_mean"], out["running_var"] = torch.from_numpy(d["rm"].copy()), torch.from_numpy(d["rv"].copy())
    # apply, f32 operation by operation
    xn = x[:n]
    v = (xn - mean_f) * invstd_f * gamma + beta
    assert v.dtype == f32
    pre = v
    if with_res:
        v = v + d["res"][:n]
    if relu:
        v = np.maximum(v, f32(0))
    out["y"] = _store(v, td)
    # backward
    y = out["y"].float().numpy() if y_given is None else y_given[:n]
    g = dy[:n]
    if relu:
        g = np.where((pre if defect == "mask_before_residual" else y) > 0, g, f32(0))
    xh = (xn - mean_f) * invstd_f
    g64 = g.astype(np.float64)
    second = xn.astype(np.float64) if defect == "dgamma_with_x" else xh.astype(np.float64)
    sa, sb = _finish(_partials(g64, g64 * second, n, G, grouping, defect))
    dbeta, dgamma = sa.astype(f32), sb.astype(f32)
    inv_n = f32(1.0) / f32(cap if defect == "inv_n_from_cap" else n) if n > 0 else f32(0)
    mean_term = f32(0) if defect == "no_mean_subtraction" else dbeta * inv_n
    dx = gamma * invstd_f * (g - mean_term - xh * dgamma * inv_n)
    assert dx.dtype == f32
    out.update(dbeta=torch.from_numpy(dbeta), dgamma=torch.from_numpy(dgamma), dx=_store(dx, td),
               dres=_store(dy[:n] if defect == "dres_unmasked" else g, td))
    return out


def inputs(C, n, cap, td, dist, seed=0, spare="same"):
    """stored inputs as f32 numpy arrays, drawn as the GPU cases draw them; the rows behind n hold NaN there ('nan') — 'same' keeps
    them in the distribution, which makes a kernel that reads them HARDER to see"""
    gen = torch.Generator().manual_seed(seed + C)
    gamma, beta, rm, rv = draw_affine(gen, C, "cpu")
    rows = min(cap, n + 3000 + C)          # (a thin frame: the capacity enters through the grid and inv_n only)
    d = dict(gamma=gamma, beta=beta, rm=rm, rv=rv, x=draw(gen, rows, C, td, dist, "cpu").float())
    for k in ("res", "dy", "yb"):
        d[k] = torch.randn(rows, C, generator=gen).to(td).float()
    if spare == "nan":
        for k in ("x", "res", "dy", "yb"):
            d[k][n:] = float("nan")
    return {k: v.numpy() for k, v in d.items()}


def reference(d, n, td, relu, with_res, y_stored, eps=EPS):
    ref = B.forward(d["x"], n, d["gamma"], d["beta"], eps, d["res"] if with_res else None, relu, d["rm"], d["rv"], MOMENTUM, td)
    ref.update(B.backward(d["dy"], d["x"], y_stored, n, d["gamma"], eps, relu, td))
    return ref


def verdict(out, ref, n):
    """{output: worst err / bound}, the names of the outputs outside their bound"""
    ratios, bad = {}, []
    for k, (V, e) in ref.items():
        worst, rep = R.check(out[k], V, e, n if V.dim() == 2 else None)
        ratios[k] = worst
        if rep is not None:
            bad.append(k)
    return ratios, bad


def judged(d, n, cap, td, relu, with_res, **kw):
    """run the emulation and hold it to the reference, the backward's mask being the y the emulation stored (or y_given)"""
    out = emulate(d, n, cap, td, relu, with_res, **kw)
    y_stored = out["y"].float() if kw.get("y_given") is None else kw["y_given"]
    return verdict(out, reference(d, n, td, relu, with_res, y_stored, kw.get("eps", EPS)), n)


# (C, n, cap), each with 256 workgroups: ~n / 256 rows per workgroup; a thin frame under the GPU case's capacity; 32 lanes per row.
# SHARE: 256 workgroups forced on a capacity with the GPU cases' share of spare rows (3 000 of 2.3 M)
SIZES = [(16, 60005, 530000), (16, 255, 1100003), (256, 9001, 9001 + 32768)]
SHARE = (16, 60005, 60005 + 80)


@pytest.mark.parametrize("td", DTYPES, ids=["f32", "bf16", "fp16"])
@pytest.mark.parametrize("dist", ["unit", "large"])
@pytest.mark.parametrize("C,n,cap", SIZES)
def test_a_correct_emulation_lies_inside_every_bound(C, n, cap, dist, td):
    assert stats_grid(cap, C) == 256
    d = inputs(C, n, cap, td, dist, spare="nan")
    for i, (relu, with_res) in enumerate(FORMS):
        for grouping in ((1, 7, 64) if i == 0 else (4,)):
            ratios, bad = judged(d, n, cap, td, relu, with_res, grouping=grouping)
            assert not bad and max(ratios.values()) < 1.0, (relu, with_res, grouping, ratios)
    ratios, bad = judged(d, n, cap, td, True, False, grouping=4, y_given=d["yb"])     # a mask of the test's own
    assert not bad and max(ratios.values()) < 1.0, ratios


def test_the_bounds_of_f32_outputs_are_tight_enough_to_matter():
    """with f32 rows an output rounded to bf16 is outside the f32 bound (the honest emulation's ratios reach 0.9 where an output's last
    step is its f32 rounding: the bound has no slack to spare there)"""
    C, n, cap = SIZES[0]
    d = inputs(C, n, cap, torch.float32, "unit")
    out = emulate(d, n, cap, torch.float32, True, True, grouping=4)
    ref = reference(d, n, torch.float32, True, True, out["y"])
    ratios, bad = verdict(out, ref, n)
    assert not bad and max(ratios.values()) < 1.0 and ratios["dgamma"] < 0.05, ratios
    with pytest.raises(R.OutOfBound):
        R.assert_within(out["y"].to(torch.bfloat16), *ref["y"], n, what="bf16 against the f32 bound")
    with pytest.raises(R.OutOfBound):
        R.assert_within(out["mean"].to(torch.bfloat16), *ref["mean"], what="bf16 mean")


# defect -> (size, form (relu, residual), the outputs that must be outside their bound, the GPU case that catches it)
THIN, CAPPED, WIDE = SIZES[1], SIZES[0], SIZES[2]
DEFECTS = {
    "lost_channel_groups": (WIDE, (True, True), ["mean", "y", "dgamma"], "test_capped_grid[256-*]"),
    "rows_to_cap": (SHARE, (True, True), ["mean"], "every case: spare rows hold NaN there; here they are in the distribution, at the same share of n"),
    "biased_running_var": (THIN, (True, True), ["running_var"], "test_thin_frames (n = 2, 17, 255): the factor n / (n - 1)"),
    "unbiased_invstd": (THIN, (True, True), ["invstd"], "test_thin_frames (n = 2, 17, 255)"),
    "momentum_reversed": (CAPPED, (True, True), ["running_mean", "running_var"], "every case with running statistics"),
    "mask_before_residual": (CAPPED, (True, True), ["dres", "dx", "dbeta"], "every relu + residual case"),
    "dres_unmasked": (CAPPED, (True, True), ["dres"], "every relu + residual case"),
    "no_mean_subtraction": (CAPPED, (True, True), ["dx"], "every case"),
    "inv_n_from_cap": (THIN, (True, True), ["dx"], "test_thin_frames: n << cap (at the capped grid cap / n - 1 is 1e-3 of a term that is 1e-3 of dx)"),
    "dgamma_with_x": (CAPPED, (True, True), ["dgamma", "dx"], "every case"),
    # 1 row of 235 per workgroup here, 1 of ~9 000 in test_capped_grid: 40 x harder there, against ratios of 10^3 and more here; the
    # rejection that does not depend on the data is test_lost_rows_and_partials_are_rejected_by_the_exact_cases
    "lost_row": (CAPPED, (True, True), ["mean", "dbeta"], "test_integer_inputs_are_exact_at_the_capped_grid; with these inputs also test_capped_grid"),
    "lost_partials": (CAPPED, (True, True), ["mean", "dbeta", "y", "dx"], "test_integer_inputs_are_exact_at_the_capped_grid; test_capped_grid"),
}


@pytest.mark.parametrize("td", DTYPES, ids=["f32", "bf16", "fp16"])
@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_every_planted_defect_is_rejected(defect, td):
    (C, n, cap), (relu, with_res), must, _where = DEFECTS[defect]
    for dist in ("unit", "large"):
        d = inputs(C, n, cap, td, dist)
        ratios, bad = judged(d, n, cap, td, relu, with_res, grouping=4)
        assert not bad, (dist, ratios)
        ratios, bad = judged(d, n, cap, td, relu, with_res, grouping=4, defect=defect)
        assert set(must) <= set(bad), (defect, dist, bad, ratios)


def test_rows_behind_n_read_into_the_statistics_show_as_nan():
    """the GPU cases fill the rows behind n with NaN: one of them in a sum and every output of the channel is NaN"""
    C, n, cap = CAPPED
    d = inputs(C, n, cap, torch.bfloat16, "unit", spare="nan")
    ratios, bad = judged(d, n, cap, torch.bfloat16, True, True, grouping=4, defect="rows_to_cap")
    assert {"mean", "invstd", "y", "dx"} <= set(bad) and ratios["mean"] == float("inf")


# ------------------------------------------------------------------------------------------------ lost rows and lost partials
@pytest.mark.parametrize("defect", ["lost_row", "lost_partials"])
def test_lost_rows_and_partials_are_rejected_by_the_exact_cases(defect):
    """The last row of every workgroup's range dropped from the statistics (256 of n rows), and the partials beyond the first 128 not
    added.  The issue behind these tests expected that random data under a rounding bound cannot show them; under the per-output
    bounds of ref64_bn it does (test_every_planted_defect_is_rejected: save_mean and dbeta are f32 roundings of f64 sums, and
    256 / n of a term is 10^3 bounds and more), but only as far as the lost rows do not happen to cancel.  The exact cases of the GPU
    file (test_integer_inputs_are_exact_at_the_capped_grid) do not depend on the data: integer inputs, sums compared bit for bit.
    Here the same inputs at 256 workgroups: the honest emulation is bit-exact, each defect is not, in mean, dbeta and dgamma."""
    C, n, cap = 16, 150038, 530000
    assert n % 2 == 0 and n % 16 and stats_grid(cap, C) == 256
    rng = np.random.default_rng(5)
    gen = torch.Generator().manual_seed(1)
    gamma, beta, rm, rv = (t.numpy() for t in draw_affine(gen, C, "cpu"))
    half = rng.integers(0, 2, (n // 2, C)) * 2 - 1
    signs = np.concatenate([half, -half, np.zeros((cap - n, C))]).astype(f32)
    ints = rng.integers(-3, 4, (cap, C)).astype(f32)
    dy, yb = rng.integers(-2, 3, (cap, C)).astype(f32), rng.integers(-1, 2, (cap, C)).astype(f32)
    for x, eps in ((ints, EPS), (signs, 3.0)):
        d = dict(x=x, dy=dy, gamma=gamma, beta=beta, rm=rm, rv=rv)
        sx, sg, sgx = B.exact_sums(x, dy, yb, n, True)
        want_mean, want_dbeta = B.f32_of_ratio(sx, n), sg.to(torch.float64).to(torch.float32)
        good = emulate(d, n, cap, torch.float32, True, False, grouping=4, y_given=yb, eps=eps)
        assert torch.equal(good["mean"], want_mean) and torch.equal(good["dbeta"], want_dbeta)
        if eps == 3.0:
            assert torch.equal(good["invstd"], torch.full((C,), 0.5)) and torch.equal(good["dgamma"], (sgx.to(torch.float64) * 0.5).to(torch.float32))
        bad = emulate(d, n, cap, torch.float32, True, False, grouping=4, y_given=yb, eps=eps, defect=defect)
        assert not torch.equal(bad["mean"], want_mean)
        assert not torch.equal(bad["dbeta"], want_dbeta)
        if eps == 3.0:
            assert not torch.equal(bad["dgamma"], (sgx.to(torch.float64) * 0.5).to(torch.float32))


def test_the_restated_grid():
    assert [stats_grid(c, 16) for c in (1, 2048, 2049, 70001 + 37, 524288 - 2048, 524288, 10 ** 7)] == [1, 1, 2, 35, 255, 256, 256]
    assert stats_grid(20000 + 37, 64) == 40 and stats_grid(5001 + 37, 128) == 20 and stats_grid(3001 + 37, 256) == 24     # the existing test's largest grids
    assert all(threshold(C) == 8388608 // C and rows_per_iter(C) * 8 == 32768 // C for C in (8, 16, 32, 64, 128, 256))
