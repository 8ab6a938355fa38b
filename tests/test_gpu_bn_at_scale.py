"""The BatchNorm training kernels (csrc/bnorm.hip: fnp_bn_train_forward / fnp_bn_train_backward, reached through spconv/norm.bn_act)
against the float64 reference of tests/ref64_bn.py AT THE CAPPED GRID: 256 statistics workgroups over contiguous row ranges and a
finishing kernel that adds 256 partials in 16 slices — the regime the training step runs them in, which no other test reaches
(the largest grid of test_fused_bn_relu_residual_matches_torch is 40).  Every element of every row below n must lie within its own
DERIVED bound (ref64_bn's docstring); there is no allowance, not at the ReLU either: the mask is `y > 0` on the y the kernel is given.
The err / bound ratios each case prints are for the record, never a criterion.

The entry points are driven through findnpropagate_amd.lib directly (and once per dtype through bn_act).  Every output buffer is
prefilled with NaN, and so are the rows of x, residual and dy behind n: a kernel that reads or writes a row it must not shows.

The row counts follow from stats_grid() of csrc/bnorm.hip, restated here: a statistics workgroup of 512 threads takes
rows_per_iter = 512 / (C / 8) rows per trip and the grid is min(256, ceil(cap / (8 * rows_per_iter))), so the cap of 256 partials is
reached from cap = 8 388 608 / C rows."""
import time

import pytest
import torch

import ref64_bn as B
from test_gpu_conv_at_scale import Recorder

pytestmark = pytest.mark.gpu

STAT_THREADS, MAX_PARTS, UNROLL = 512, 256, 4       # kStatThreads, kMaxParts, kUnroll
FNP_ERR_ARG, FNP_ERR_WORKSPACE = -1, -4
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "fp16"]
EPS, MOMENTUM = 1e-3, 0.01


def rows_per_iter(C):
    return STAT_THREADS // (C // 8)


def stats_grid(cap, C, capped=True):
    g = -(-cap // (rows_per_iter(C) * 8))
    return max(1, min(g, MAX_PARTS) if capped else g)


def threshold(C):
    """the capacity from which the grid is capped"""
    return MAX_PARTS * 8 * rows_per_iter(C)


assert [threshold(C) for C in (8, 16, 32, 64, 128, 256)] == [1048576, 524288, 262144, 131072, 65536, 32768]


def n_for(C, factor=2.2):
    """rows for `factor` times the threshold: not a multiple of 16, so of neither rows_per_iter nor U * rows_per_iter"""
    n = int(factor * threshold(C)) // 16 * 16 + 5
    assert n % 16 and n % rows_per_iter(C) and n % (UNROLL * rows_per_iter(C)) and n % (UNROLL // 2 * rows_per_iter(C))
    return n


# ------------------------------------------------------------------------------------------------ inputs
def draw(gen, cap, C, td, dist, device):
    """x (cap, C) in td.  'unit': the distribution of test_fused_bn_relu_residual_matches_torch (scale 1.7 plus a per-channel offset
    of order one); 'large': per-channel means of +-(200 .. 400) with a standard deviation of order one — the feature scale VERDICT
    reports (200 - 340), where a statistics pass that is not in f64 fails."""
    r = lambda *s: torch.randn(*s, generator=gen, device=device)
    if dist == "unit":
        x = r(cap, C) * 1.7 + r(C)
    else:
        off = (200.0 + 200.0 * torch.rand(C, generator=gen, device=device)) * torch.sign(r(C))
        x = r(cap, C) + off
    return x.to(td)


def draw_affine(gen, C, device):
    gamma = 0.5 + torch.rand(C, generator=gen, device=device)
    return gamma, torch.randn(C, generator=gen, device=device), torch.randn(C, generator=gen, device=device), 0.5 + torch.rand(C, generator=gen, device=device)


def _nan_behind(t, n):
    t[n:] = float("nan")
    return t


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ------------------------------------------------------------------------------------------------ the two entry points
def _lib():
    from findnpropagate_amd import lib
    return lib, lib.load()


def _ws(C, cuda):
    lib, L = _lib()
    return torch.empty((int(L.fnp_bn_workspace_bytes(C)),), dtype=torch.uint8, device=cuda)


def _nan(shape, dtype, cuda):
    return torch.full(shape, float("nan"), dtype=dtype, device=cuda)


def bn_forward(x, n_dev, cap, gamma, beta, rm, rv, residual, relu, nbt, eps=EPS, momentum=MOMENTUM, expect=0, C=None, ws_short=0, out=None):
    """-> y, save_mean, save_invstd (NaN-prefilled) after fnp_bn_train_forward"""
    lib, L = _lib()
    C = x.shape[1] if C is None else C
    cuda = x.device
    y, mean, invstd = out or (_nan(tuple(x.shape), x.dtype, cuda), _nan((x.shape[1],), torch.float32, cuda), _nan((x.shape[1],), torch.float32, cuda))
    ws = _ws(max(C, 8), cuda)
    rc = L.fnp_bn_train_forward(lib.ptr(x), lib.dtype_code(x), lib.ptr(n_dev), cap, C, lib.ptr(gamma), lib.ptr(beta), lib.ptr(rm), lib.ptr(rv),
                                float(momentum), float(eps), lib.ptr(residual), int(relu), lib.ptr(y), lib.ptr(mean), lib.ptr(invstd), lib.ptr(nbt),
                                lib.ptr(ws), int(L.fnp_bn_workspace_bytes(C)) - ws_short, lib.stream())
    assert rc == expect, (rc, expect)
    torch.cuda.synchronize()
    return y, mean, invstd


def bn_backward(dy, x, y, n_dev, cap, gamma, mean, invstd, relu, want_dres, expect=0, C=None, ws_short=0):
    """-> dx, dres or None, dgamma, dbeta (NaN-prefilled) after fnp_bn_train_backward"""
    lib, L = _lib()
    C = x.shape[1] if C is None else C
    cuda = x.device
    dx = _nan(tuple(x.shape), x.dtype, cuda)
    dres = _nan(tuple(x.shape), x.dtype, cuda) if want_dres else None
    dgamma, dbeta = _nan((x.shape[1],), torch.float32, cuda), _nan((x.shape[1],), torch.float32, cuda)
    ws = _ws(max(C, 8), cuda)
    rc = L.fnp_bn_train_backward(lib.ptr(dy), lib.ptr(x), lib.ptr(y), lib.dtype_code(x), lib.ptr(n_dev), cap, C, lib.ptr(gamma), lib.ptr(mean),
                                 lib.ptr(invstd), int(relu), lib.ptr(dx), lib.ptr(dres), lib.ptr(dgamma), lib.ptr(dbeta), lib.ptr(ws),
                                 int(L.fnp_bn_workspace_bytes(C)) - ws_short, lib.stream())
    assert rc == expect, (rc, expect)
    torch.cuda.synchronize()
    return dx, dres, dgamma, dbeta


def _untouched(rec, name, t, n):
    """rows at and behind n still hold the NaN prefill"""
    if t is not None and not bool(torch.isnan(t[n:]).all()):
        rec.fail.append(f"{name}: rows at or behind n = {n} were written")


# (name, relu, residual, running statistics, num_batches_tracked, grad_residual, the y the backward is given)
FORMS = [("relu+res", True, True, True, True, True, "own"),
         ("relu", True, False, False, False, False, "built"),
         ("res", False, True, True, False, False, "null"),
         ("plain", False, False, False, True, False, "own")]


class Case:
    """the inputs of one (C, n, cap, dtype) on the device, NaN behind n, with their statistics in float64"""

    def __init__(self, rec, cuda, C, n, cap, td, dists=("unit", "large"), seed=11):
        from findnpropagate_amd import sparse as S
        self.rec, self.cuda, self.C, self.n, self.cap, self.td = rec, cuda, C, n, cap, td
        gen = torch.Generator(device=cuda).manual_seed(seed + C)
        self.gamma, self.beta, self.rm0, self.rv0 = draw_affine(gen, C, cuda)
        self.x = {d: _nan_behind(draw(gen, cap, C, td, d, cuda), n) for d in dists}
        self.res = _nan_behind(torch.randn(cap, C, generator=gen, device=cuda).to(td), n)
        self.dy = _nan_behind(torch.randn(cap, C, generator=gen, device=cuda).to(td), n)
        self.y_built = _nan_behind(torch.randn(cap, C, generator=gen, device=cuda).to(td), n)     # a mask of the test's own
        self.n_dev = S.device_scalar(n, cuda)
        t0 = time.perf_counter()
        self.st = {d: B.stats(self.x[d], n, EPS) for d in dists}
        rec.t_ref += time.perf_counter() - t0

    def run(self, form, dist, twice=False, n_dev=None, n=None):
        name, relu, with_res, running, tracked, want_dres, y_src = form
        rec, cuda, C, cap = self.rec, self.cuda, self.C, self.cap
        n = self.n if n is None else n
        x, st = self.x[dist], self.st[dist]
        res = self.res if with_res else None
        tag = f"{name} {dist}"

        def once():
            rm, rv = (self.rm0.clone(), self.rv0.clone()) if running else (None, None)
            nbt = torch.full((1,), 41, dtype=torch.int64, device=cuda) if tracked else None
            y, mean, invstd = bn_forward(x, n_dev if n_dev is not None else self.n_dev, cap, self.gamma, self.beta, rm, rv, res, relu, nbt)
            if tracked and int(nbt.item()) != 42:
                rec.fail.append(f"{tag}: num_batches_tracked {int(nbt.item())}, not 42")
            y_bwd = {"own": y, "built": self.y_built, "null": None}[y_src]
            dx, dres, dgamma, dbeta = bn_backward(self.dy, x, y_bwd, n_dev if n_dev is not None else self.n_dev, cap, self.gamma, mean, invstd, relu,
                                                  want_dres)
            return dict(y=y, mean=mean, invstd=invstd, running_mean=rm, running_var=rv, dx=dx, dres=dres, dgamma=dgamma, dbeta=dbeta), y_bwd

        got, y_bwd = once()
        t0 = time.perf_counter()
        ref = B.forward(x, n, self.gamma, self.beta, EPS, res, relu, self.rm0 if running else None, self.rv0 if running else None, MOMENTUM,
                        self.td, st=st)
        rec.t_ref += time.perf_counter() - t0
        for k in ("mean", "invstd", "running_mean", "running_var"):
            if k in ref:
                rec.check(f"{tag} | {k}", got[k], *ref[k], None, None)
        if n:
            rec.check(f"{tag} | y", got["y"], *ref["y"], n, None)
        del ref
        t0 = time.perf_counter()
        ref = B.backward(self.dy, x, y_bwd, n, self.gamma, EPS, relu, self.td, st=st)
        rec.t_ref += time.perf_counter() - t0
        for k in ("dbeta", "dgamma"):
            rec.check(f"{tag} | {k}", got[k], *ref[k], None, None)
        if n:
            rec.check(f"{tag} | dx", got["dx"], *ref["dx"], n, None)
            if want_dres:
                rec.check(f"{tag} | dres", got["dres"], *ref["dres"], n, None)
        del ref
        for k in ("y", "dx", "dres"):
            _untouched(rec, f"{tag} | {k}", got[k], n)
        if twice:       # a second run on the same inputs: the same bits in every output
            again, _ = once()
            for k, t in got.items():
                if t is not None and not torch.equal(_bits(t), _bits(again[k])):
                    rec.fail.append(f"{tag} | {k}: a second run gave other bits")
        return got


# ------------------------------------------------------------------------------------------------ the capped grid
@pytest.mark.parametrize("td", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [8, 16, 32, 64, 128, 256])
def test_capped_grid(cuda, C, td):
    """n = 2.2 x the threshold (18.4 M elements per tensor): 256 workgroups of ~n / 256 contiguous rows, several trips of U rows each and
    a partial one, 256 partials into the finishing kernel.  All four (relu, residual) forms in both directions; the options
    (running statistics, num_batches_tracked, grad_residual, the backward's y) change with the form (FORMS); the two distributions
    change places from one C to the next; the first form runs twice."""
    n, spare = n_for(C), 3000 + C
    cap = n + spare
    assert stats_grid(cap, C) == MAX_PARTS and stats_grid(cap, C, capped=False) >= 2 * MAX_PARTS and stats_grid(n, C) == MAX_PARTS
    per = -(-n // MAX_PARTS)
    assert per > 2 * UNROLL * rows_per_iter(C) and per * (MAX_PARTS - 1) < n       # every workgroup has rows; several full trips each
    rec = Recorder(f"bn capped grid C={C} n={n} cap={cap} {td}")
    case = Case(rec, cuda, C, n, cap, td)
    flip = [8, 16, 32, 64, 128, 256].index(C) % 2
    for i, form in enumerate(FORMS):
        case.run(form, ("unit", "large")[(i // 2 + flip) % 2], twice=(i == 0))
    rec.done()


@pytest.mark.parametrize("td", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [16, 128])
@pytest.mark.parametrize("side", ["below", "above"])
def test_both_sides_of_the_256_partial_threshold(cuda, side, C, td):
    """cap one workgroup's share (8 * rows_per_iter rows) below the threshold: 255 workgroups, 15 finishing slices of 16 partials and
    one of 15; one share above: 256, where the uncapped count would be 257"""
    share = 8 * rows_per_iter(C)
    cap = threshold(C) + (share if side == "above" else -share)
    n = cap - 16 - 11
    assert n % 16 and stats_grid(cap, C) == (256 if side == "above" else 255) and stats_grid(cap, C, capped=False) == (257 if side == "above" else 255)
    rec = Recorder(f"bn threshold {side} C={C} n={n} cap={cap} {td}")
    case = Case(rec, cuda, C, n, cap, td, seed=23)
    case.run(FORMS[0], "large" if side == "above" else "unit")
    case.run(FORMS[3], "unit" if side == "above" else "large")
    rec.done()


# (C, rows, the grid it reaches, where the figure is recorded).  The 16-scene figures are the stage rows of tools/ab_bnorm.py; the
# 4 x 10-sweep step has 480 k voxels at 16 channels (the 120 k cap fires on each of the 4 scenes).  Its rows
# at 32, 64 and 128 channels are recorded nowhere: 3 x the threshold stands in for them.
STAGE_ROWS = [(16, 480000, 236, "4 x 10 sweeps"), (16, 301444, 149, "16 scenes"), (32, 560000, 256, "16 scenes"), (64, 330000, 256, "16 scenes"),
              (128, 136000, 256, "16 scenes"), (32, 3 * 262144 + 5, 256, "3 x threshold"), (64, 3 * 131072 + 5, 256, "3 x threshold"),
              (128, 3 * 65536 + 5, 256, "3 x threshold")]


@pytest.mark.parametrize("C,n,grid,what", STAGE_ROWS)
def test_stage_row_counts_of_the_training_step(cuda, C, n, grid, what):
    """the row counts of the backbone's stages in the 16-scene and the 4 x 10-sweep training step, fp16 as under autocast, in the two
    forms the backbone uses (BatchNorm + ReLU, with and without the residual)"""
    td = torch.float16
    cap = n + 3000
    assert stats_grid(cap, C) == grid
    rec = Recorder(f"bn stage rows ({what}) C={C} n={n} cap={cap} grid={grid} {td}")
    case = Case(rec, cuda, C, n, cap, td, seed=37)
    case.run(FORMS[0], "unit")
    case.run(FORMS[1], "large")
    rec.done()


# ------------------------------------------------------------------------------------------------ thin frames
@pytest.mark.parametrize("td", DTYPES, ids=IDS)
def test_thin_frames_under_a_fixed_capacity(cuda, td):
    """a replayed graph's fixed capacity with a thin frame: n in {0, 1, 2, 17, 255} under 1.1 M rows of capacity at 16 channels (256
    workgroups, all but the first few without a row), and *n_rows ABOVE the capacity, which the kernels clamp.  Rows at and behind n
    keep the NaN they were prefilled with; n = 0 leaves the running statistics as they were."""
    from findnpropagate_amd import sparse as S
    C, cap = 16, 1100003
    assert stats_grid(cap, C) == MAX_PARTS
    rec = Recorder(f"bn thin frames C={C} cap={cap} {td}")
    for n_rows in (0, 1, 2, 17, 255, cap + 12345):
        n = min(n_rows, cap)
        case = Case(rec, cuda, C, n, cap, td, dists=("unit",) if n == cap else ("unit", "large"), seed=5 + n % 1000)
        n_dev = S.device_scalar(n_rows, cuda)
        got = case.run(("n_rows=%d %s" % (n_rows, FORMS[0][0]),) + FORMS[0][1:], "unit", n_dev=n_dev, n=n)
        if n == 0:
            assert torch.equal(got["running_mean"], case.rm0) and torch.equal(got["running_var"], case.rv0)
            assert float(got["mean"].abs().max()) == 0.0 and torch.equal(got["dbeta"], torch.zeros_like(got["dbeta"]))
        if n < cap:
            case.run(("n_rows=%d %s" % (n_rows, FORMS[3][0]),) + FORMS[3][1:], "large", n_dev=n_dev, n=n)
        del case
    rec.done()


# ------------------------------------------------------------------------------------------------ exact cases: bound zero
@pytest.mark.parametrize("td", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [16, 64, 256])
def test_integer_inputs_are_exact_at_the_capped_grid(cuda, C, td):
    """Integer x and dy: every f64 sum is exact whatever its order, so save_mean must be float32(sum x / n) and dbeta float32(sum g) BIT
    FOR BIT — one lost row, one lost partial or one row counted twice shows, which no rounding bound at 2 * 10^6 rows promises for
    every input.  Then x in {-1, +1} with equal counts per channel and eps = 3: mean = 0, var = 1, invstd = 0.5 exactly, xhat = x / 2
    is exact in f32, the terms of dgamma are multiples of 0.5 and dgamma is bit-exact too."""
    from findnpropagate_amd import sparse as S
    n = n_for(C) + 1
    cap = n + 3000
    assert n % 2 == 0 and n % 16 and stats_grid(cap, C) == MAX_PARTS
    rec = Recorder(f"bn exact C={C} n={n} cap={cap} {td}")
    gen = torch.Generator(device=cuda).manual_seed(77 + C)
    ri = lambda lo, hi, rows=cap: torch.randint(lo, hi, (rows, C), generator=gen, device=cuda).to(td)
    gamma, beta, _, _ = draw_affine(gen, C, cuda)
    n_dev = S.device_scalar(n, cuda)
    dy, y_built = _nan_behind(ri(-2, 3), n), _nan_behind(ri(-1, 2), n)
    half = ri(0, 2, n // 2) * 2 - 1
    signs = _nan_behind(torch.cat([half, -half, torch.zeros((cap - n, C), dtype=td, device=cuda)]), n)
    for name, x, eps in (("integers", _nan_behind(ri(-3, 4), n), EPS), ("signs", signs, 3.0)):
        for relu in (True, False):
            y, mean, invstd = bn_forward(x, n_dev, cap, gamma, beta, None, None, None, relu, None, eps=eps)
            dx, _, dgamma, dbeta = bn_backward(dy, x, y_built if relu else None, n_dev, cap, gamma, mean, invstd, relu, False)
            t0 = time.perf_counter()
            sx, sg, sgx = B.exact_sums(x.cpu().float(), dy.cpu().float(), y_built.cpu().float(), n, relu)
            rec.t_ref += time.perf_counter() - t0
            zero = torch.zeros(1, dtype=torch.float64)
            tag = f"{name} relu={int(relu)}"
            rec.check(f"{tag} | mean", _bits(mean), _bits(B.f32_of_ratio(sx, n)).double(), zero, None, None)
            rec.check(f"{tag} | dbeta", _bits(dbeta), _bits(sg.to(torch.float64).to(torch.float32)).double(), zero, None, None)
            if name == "signs":
                assert int(sx.abs().max()) == 0
                rec.check(f"{tag} | invstd", _bits(invstd), _bits(torch.full((C,), 0.5)).double(), zero, None, None)
                rec.check(f"{tag} | dgamma", _bits(dgamma), _bits((sgx.to(torch.float64) * 0.5).to(torch.float32)).double(), zero, None, None)
            _untouched(rec, f"{tag} | y", y, n)
            _untouched(rec, f"{tag} | dx", dx, n)
            if bool(torch.isnan(y[:n]).any()) or bool(torch.isnan(dx[:n]).any()):
                rec.fail.append(f"{tag}: NaN below n")
    rec.done()


# ------------------------------------------------------------------------------------------------ through bn_act
@pytest.mark.parametrize("td", DTYPES, ids=IDS)
def test_bn_act_at_the_capped_grid(cuda, td):
    """the autograd node of spconv/norm.py on a BatchNorm1d module at 64 channels, 2.2 x the threshold: output, the four gradients,
    the running statistics and num_batches_tracked (int64 on the device: advanced by the kernel)"""
    from findnpropagate_amd import sparse as S
    from findnpropagate_amd.spconv import norm as N
    C = 64
    n, cap = n_for(C), n_for(C) + 3000
    assert stats_grid(cap, C) == MAX_PARTS
    rec = Recorder(f"bn_act C={C} n={n} cap={cap} {td}")
    gen = torch.Generator(device=cuda).manual_seed(3)
    gamma, beta, rm0, rv0 = draw_affine(gen, C, cuda)
    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=MOMENTUM).to(cuda).train()
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm0), bn.running_var.copy_(rv0)
    assert bn.num_batches_tracked.is_cuda and bn.num_batches_tracked.dtype == torch.int64
    x0 = draw(gen, cap, C, td, "large", cuda)
    r0 = torch.randn(cap, C, generator=gen, device=cuda).to(td)
    dy = torch.randn(cap, C, generator=gen, device=cuda).to(td)
    n_dev = S.device_scalar(n, cuda)
    for step in (1, 2):
        rm_before, rv_before = bn.running_mean.clone(), bn.running_var.clone()
        x, r = x0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
        bn.zero_grad()
        y = N.bn_act(x, n_dev, bn, residual=r, relu=True)
        assert y.dtype == td
        (y[:n].float() * dy[:n].float()).sum().backward()
        torch.cuda.synchronize()
        assert int(bn.num_batches_tracked.item()) == step
        t0 = time.perf_counter()
        ref = B.forward(x0, n, gamma, beta, EPS, r0, True, rm_before, rv_before, MOMENTUM, td)
        rec.t_ref += time.perf_counter() - t0
        rec.check(f"step {step} | y", y.detach(), *ref["y"], n, None)
        rec.check(f"step {step} | running_mean", bn.running_mean, *ref["running_mean"], None, None)
        rec.check(f"step {step} | running_var", bn.running_var, *ref["running_var"], None, None)
        del ref
        t0 = time.perf_counter()
        ref = B.backward(dy, x0, y.detach(), n, gamma, EPS, True, td)
        rec.t_ref += time.perf_counter() - t0
        rec.check(f"step {step} | dx", x.grad, *ref["dx"], n, None)
        rec.check(f"step {step} | dres", r.grad, *ref["dres"], n, None)
        rec.check(f"step {step} | dgamma", bn.weight.grad, *ref["dgamma"], None, None)
        rec.check(f"step {step} | dbeta", bn.bias.grad, *ref["dbeta"], None, None)
        del ref
    rec.done()


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
def test_argument_and_workspace_errors_launch_nothing(cuda):
    """FNP_ERR_ARG for a channel count that is not a power of two in 8 .. 256, cap = 0, exactly one of the running statistics, relu
    without y in the backward; FNP_ERR_WORKSPACE for a workspace one byte short.  None of them may launch anything: every output
    still holds its NaN prefill afterwards, num_batches_tracked and the running statistics are as they were."""
    from findnpropagate_amd import sparse as S
    C, cap, n = 16, 64, 50
    gen = torch.Generator(device=cuda).manual_seed(1)
    gamma, beta, rm0, rv0 = draw_affine(gen, C, cuda)
    n_dev = S.device_scalar(n, cuda)
    for td in DTYPES:
        x, dy = draw(gen, cap, C, td, "unit", cuda), draw(gen, cap, C, td, "unit", cuda)
        mean, invstd = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
        rm, rv = rm0.clone(), rv0.clone()
        nbt = torch.full((1,), 7, dtype=torch.int64, device=cuda)
        outs = []
        fwd = lambda **kw: outs.extend(bn_forward(x, n_dev, kw.pop("cap", cap), gamma, beta, kw.pop("rm", rm), kw.pop("rv", rv), None, True, nbt, **kw))
        bwd = lambda **kw: outs.extend(t for t in bn_backward(dy, x, kw.pop("y", x), n_dev, kw.pop("cap", cap), gamma, mean, invstd, kw.pop("relu", True),
                                                              True, **kw) if t is not None)
        for bad_c in (24, 4, 512, 0, -16):
            fwd(C=bad_c, expect=FNP_ERR_ARG)
            bwd(C=bad_c, expect=FNP_ERR_ARG)
        for bad_cap in (0, -5):
            fwd(cap=bad_cap, expect=FNP_ERR_ARG)
            bwd(cap=bad_cap, expect=FNP_ERR_ARG)
        fwd(rm=None, expect=FNP_ERR_ARG)
        fwd(rv=None, expect=FNP_ERR_ARG)
        bwd(y=None, relu=True, expect=FNP_ERR_ARG)
        fwd(ws_short=1, expect=FNP_ERR_WORKSPACE)
        bwd(ws_short=1, expect=FNP_ERR_WORKSPACE)
        torch.cuda.synchronize()
        assert len(outs) == 10 * 3 + 9 * 4
        assert all(bool(torch.isnan(t).all()) for t in outs), "an entry point that refused its arguments wrote an output"
        assert int(nbt.item()) == 7 and torch.equal(rm, rm0) and torch.equal(rv, rv0)
        # and the same buffers are accepted once the arguments are right (relu = 0 takes a NULL y)
        y, mean, invstd = bn_forward(x, n_dev, cap, gamma, beta, rm, rv, None, False, nbt)
        dx, dres, dgamma, dbeta = bn_backward(dy, x, None, n_dev, cap, gamma, mean, invstd, False, True)
        assert int(nbt.item()) == 8 and not bool(torch.isnan(y[:n]).any()) and bool(torch.isnan(y[n:]).all())
        assert not bool(torch.isnan(dx[:n]).any()) and torch.equal(dres[:n], dy[:n]) and not bool(torch.isnan(dgamma).any() | torch.isnan(dbeta).any())
