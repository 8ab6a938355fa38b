"""BaseBEVBackbone.first_block_from_sparse — the (D, 3, 3) stride-1 rulebook, the run-time-K matrix kernels with f32 output,
BatchNorm epilogue and ReLU (K = 18 walked in pairs, K = 9 with an odd tail), and the dense writer with a per-channel background —
against the float64 reference of tests/ref_bev.py under the DERIVED bound of tests/ref64.py (bf16 / fp16 rows) and tests/ref32.py
(f32 rows), AT THE SIZES THE BENCHMARK RUNS IT: batch 8 of (2, 180, 180) is two rounds of the 128 -> 128 persistent grid and a
partial one, under a capacity above the full-tile threshold of both kernels.  Every other test of this path compares with torch's
own f32 conv2d at 1e-4 / 2e-2 of the map's maximum and stops below one round.

Per case (the site sets of ref_bev.CASES; what each reaches is asserted on the CPU in tests/test_ref_bev.py): every output site's
128 values lie within their own bound of the reference — no allowance, no skipped element —, every other cell is max(shift, 0) of
the f32 fold bit for bit, and the rulebook equals the coordinate-derived table of tests/ref_index.py row for row in rank order with
nothing written behind it.  The err / bound ratios and times each case prints are for the record, never a criterion."""
import time

import numpy as np
import pytest
import torch

import ref64 as R
import ref_bev as RB
import ref_index as RI
from findnpropagate_amd import lib as _l
from findnpropagate_amd import sparse as S
from findnpropagate_amd import spconv
from findnpropagate_amd.backbones_2d import BaseBEVBackbone
from test_gpu_bev import CFG
from test_gpu_conv_at_scale import Recorder
from test_gpu_index_at_scale import build, check_strided, strided

pytestmark = pytest.mark.gpu

F32, BF16, FP16 = torch.float32, torch.bfloat16, torch.float16
TYPES = pytest.mark.parametrize("td", [F32, BF16, FP16], ids=["f32", "bf16", "fp16"])
TILE = 384       # rows of a workgroup tile of both 128 -> 128 kernels (ref64.check's report names the 16-row block within it)


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _module(cuda, D, **extra):
    """the backbone with 128 * D input channels, BatchNorm statistics drawn as tests/test_gpu_bev.py's `_net` draws them (channels
    of both signs of shift) and the first convolution's weight drawn without magnitudes a 16-bit type would hold as subnormals"""
    rng = np.random.default_rng(1234)
    net = BaseBEVBackbone(dict(CFG, **extra), 128 * D).to(cuda).eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, m.num_features).astype(np.float32)))
                m.bias.copy_(torch.from_numpy(rng.standard_normal(m.num_features).astype(np.float32) * 0.3))
                m.running_mean.copy_(torch.from_numpy(rng.standard_normal(m.num_features).astype(np.float32) * 0.2))
                m.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, m.num_features).astype(np.float32)))
        conv = net.blocks[0][1]
        bound = 1.0 / np.sqrt(9.0 * conv.in_channels)       # (the range of torch's default initialisation, drawn here: no global seed)
        conv.weight.copy_(torch.from_numpy(RB.stable_weight(rng.uniform(-bound, bound, tuple(conv.weight.shape)).astype(np.float32))))
    shift = RB.folded(net.blocks[0][2]).shift
    assert (shift < 0).sum() >= 8 and (shift > 0).sum() >= 8, "channels of both signs of shift"
    return net


# ------------------------------------------------------------------------------------------------ references (once per process)
_RANKED, _REFS = {}, {}


def ranked(name):
    """(output sites IN RANK ORDER, output shape, table over them, for each of them its row in ref_bev.table(name)): ref_index's and
    ref64's coordinate-derived tables, which share no code, name the same sites and the same neighbours"""
    if name not in _RANKED:
        idx, B, shape = RB.sites(name)
        out, osh, nbr = RI.neighbours_strided(idx, B, list(shape), RB.KSIZE(shape[0]), RB.STRIDE, RB.PAD)
        out64, nbr64 = RB.table(name)
        order = R.match_rows(out64, out, osh)
        assert np.array_equal(nbr64[:, order], nbr)
        _RANKED[name] = (out, osh, nbr, order)
    return _RANKED[name]


class Ref:
    pass


def reference(rec, net, name, td, x=None, cache=True):
    """the reference of a case in `td` for the module's present constants, its rows in the device's (rank) order"""
    conv, bn = net.blocks[0][1], net.blocks[0][2]
    w2d = conv.weight.detach().cpu().numpy()
    fold = RB.folded(bn)
    key = (name, td)
    if cache and x is None and key in _REFS:
        r = _REFS[key]
        assert np.array_equal(r.w2d, w2d) and np.array_equal(r.fold.scale, fold.scale) and np.array_equal(r.fold.shift, fold.shift)
        return r
    idx, B, shape = RB.sites(name)
    t0 = time.perf_counter()
    out, osh, nbr, order = ranked(name)
    r = Ref()
    r.x = RB.draw_rows(name, td) if x is None else x
    _, V, e = RB.rows_reference(idx, r.x, B, shape, RB.weight3d(w2d, shape[0]), fold.scale, fold.shift, td, tab=RB.table(name))
    o = torch.from_numpy(order)
    r.out, r.V, r.e, r.fold, r.w2d = out, V[o], e[o], fold, w2d
    rec.t_ref += time.perf_counter() - t0
    if cache and x is None:
        _REFS[key] = r
    return r


def run(net, name, td, x, cuda):
    idx, B, shape = RB.sites(name)
    feats = _dev(x, cuda).to(td)
    assert feats.dtype == td and feats.shape == (idx.shape[0], 128)
    t = spconv.SparseConvTensor(feats, _dev(idx, cuda), list(shape), B)
    with torch.no_grad():
        dense = net.first_block_from_sparse(t)
    assert dense.is_contiguous() and dense.dtype == F32 and tuple(dense.shape) == (B, 128, shape[1], shape[2])
    return dense


def check(rec, path, dense, r):
    worst, fail = RB.check_dense(dense.cpu().numpy(), r.out, r.V, r.e, r.fold.background, TILE)
    print(f"RATIO {rec.case} | {path} | {worst:.4g}")
    rec.fail += [f"{path}: {m}" for m in fail]


# ------------------------------------------------------------------------------------------------ (a) rulebook geometry
@pytest.mark.parametrize("name", list(RB.CASES))
def test_rulebook_of_the_stride_1_window(cuda, name):
    """fnp_rulebook_strided at (D, 3, 3), stride 1, pad (0, 1, 1) under the caller's tight capacity, buffers prefilled with -2 and
    slack words behind them: output sites in rank order, the table, out_n, the output grid's words"""
    idx, B, shape = RB.sites(name)
    D, H, W = shape
    n = idx.shape[0]
    out, osh, nbr, _ = ranked(name)
    cap_out = RB.cap_out_of(n, B, H, W)
    geom = (RB.KSIZE(D), RB.STRIDE, RB.PAD)
    print(f"\nFORM {name} | B {B} shape {list(shape)} | n {n} | K {nbr.shape[0]} | out_n {out.shape[0]} | cap_out {cap_out}")
    assert out.shape[0] <= cap_out and osh == [1, H, W]
    idx_dev, n_dev = _dev(idx, cuda), S.device_scalar(n, cuda)
    grid, _ = build(idx_dev, n_dev, B, list(shape), keep_order=True)        # (rows in random order: the table names rows through perm)
    s = strided(idx_dev, n_dev, grid, geom, cap_out)
    check_strided(f"{name} k{D}33 s1 p011", s, out, osh, nbr, RI.grid_words(out, B, osh))
    # ... and the entry the module calls hands out the same rows
    rb = S.rulebook_strided(idx_dev, n_dev, grid, *geom, cap_out)
    m = out.shape[0]
    assert int(rb.out_n.item()) == m and rb.K == D * 9 and rb.cap_out == cap_out
    assert torch.equal(rb.out_indices[:m], s.out_idx[:m]) and torch.equal(rb.nbr[:, :m], s.nbr[:, :m])


# ------------------------------------------------------------------------------------------------ (b) rows and placement
@TYPES
@pytest.mark.parametrize("name", list(RB.CASES))
def test_first_block_rows_and_placement(cuda, name, td):
    """net.first_block_from_sparse(t) on every site set: the rows on their sites within the bound, max(shift, 0) everywhere else"""
    idx, B, shape = RB.sites(name)
    D, H, W = shape
    rec = Recorder(f"bev {name} B={B} {list(shape)} n={idx.shape[0]} {str(td)[6:]}")
    net = _module(cuda, D)
    r = reference(rec, net, name, td)
    tc = RB.tile_classes(r.out, B, H, W)
    print(f"FORM {rec.case} | K {D * 9} | out_n {r.out.shape[0]} | cap_out {RB.cap_out_of(idx.shape[0], B, H, W)} | writer tiles of {tc['tile']} cells: "
          f"{tc['empty']} empty, {tc['slots']} of 1 .. 64, {tc['over']} above 64{', last of a plane partial' if tc['partial'] else ''}")
    t0 = time.perf_counter()
    dense = run(net, name, td, r.x, cuda)
    torch.cuda.synchronize()
    print(f"TIME {rec.case} | device call (first of its shapes, with allocations) {1e3 * (time.perf_counter() - t0):.1f} ms")
    check(rec, "first block", dense, r)
    if name == "mid" and td == F32:
        # one scene by the other route (torch's float64 conv2d on the dense map): the weight mapping, the channel order c * D + z
        # and the borders at 180 x 180, with the module's own weight — the float64 fold on both sides, to float64 rounding
        t0 = time.perf_counter()
        one = idx[:, 0] == 0
        conv, bn = net.blocks[0][1], net.blocks[0][2]
        o1, V1, _ = RB.rows_reference(idx[one], r.x[one], 1, shape, RB.weight3d(conv.weight, D), r.fold.scale64, r.fold.shift64, F32)
        a = torch.from_numpy(RB.scatter(o1, V1.numpy(), r.fold.background64, 1, H, W))
        b = RB.dense_reference(idx[one], r.x[one], 1, shape, conv.weight, bn)
        rec.t_ref += time.perf_counter() - t0
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    rec.done()


# ------------------------------------------------------------------------------------------------ (c) constants and packing
@TYPES
@pytest.mark.parametrize("D", [1, 2])
def test_prepared_constants_and_weight(cuda, D, td):
    net = _module(cuda, D)
    conv, bn = net.blocks[0][1], net.blocks[0][2]
    w, scale, shift, background = net._prepare(D, td)
    f = RB.folded(bn)
    bits = lambda a: np.ascontiguousarray(a).view(np.int32)
    for what, got, want in (("scale", scale, f.scale), ("shift", shift, f.shift), ("background", background, f.background)):
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), what
    u4 = 4 * 2.0 ** -24
    assert (np.abs(scale.cpu().numpy() - f.scale64) <= u4 * np.abs(f.scale64)).all()
    assert (np.abs(shift.cpu().numpy() - f.shift64) <= u4 * f.bias_mag).all()
    want = RB.weight3d(conv.weight, D)
    assert w.dtype == td and tuple(w.shape) == (D * 9, 128, 128) and w.is_contiguous()
    if td == F32:
        assert isinstance(w, S.PermutedWeight)
        assert np.array_equal(bits(RB.unpermute(w.as_subclass(torch.Tensor).cpu().numpy())), bits(want))
    else:
        assert np.array_equal(bits(w.float().cpu().numpy()), bits(R.round16(want, td)))
    assert net._prepare(D, td)[0] is w, "the prepared constants are cached while the parameters stand"


# ------------------------------------------------------------------------------------------------ (d) cache and casts
@TYPES
def test_parameters_changed_in_place_are_seen(cuda, td):
    """running_var, then the weight, changed in place between calls: each next call meets the reference of the new values"""
    name = "isolated"
    rec = Recorder(f"bev cache {name} {str(td)[6:]}")
    net = _module(cuda, 2)
    conv, bn = net.blocks[0][1], net.blocks[0][2]
    x = RB.draw_rows(name, td)
    prev = None
    for step in ("as built", "running_var * 1.5", "weight * 0.5"):
        with torch.no_grad():
            if step == "running_var * 1.5":
                bn.running_var.mul_(1.5)
            elif step == "weight * 0.5":
                conv.weight.mul_(0.5)     # (a power of two: the magnitudes stay clear of fp16's subnormals)
        dense = run(net, name, td, x, cuda)
        check(rec, step, dense, reference(rec, net, name, td, x=x))
        assert prev is None or not torch.equal(prev, dense), step
        prev = dense.clone()
    rec.done()


@pytest.mark.parametrize("rows,cast", [(F32, "bf16"), (BF16, "fp32")], ids=["f32-rows-as-bf16", "bf16-rows-as-fp32"])
def test_cast_of_the_rows(cuda, rows, cast):
    """FNP_BEV_DTYPE 'bf16' on f32 rows: the bf16 reference of the rounded rows; 'fp32' on bf16 rows: the f32 reference of the
    widened rows (and the unrounded weight)"""
    name = "d1-odd"
    rec = Recorder(f"bev cast {name} rows {str(rows)[6:]} FNP_BEV_DTYPE={cast}")
    net = _module(cuda, 1, FNP_BEV_DTYPE=cast)
    x = RB.draw_rows(name, rows)
    compute = {"bf16": BF16, "fp32": F32}[cast]
    dense = run(net, name, rows, x, cuda)
    check(rec, f"computed in {cast}", dense, reference(rec, net, name, compute, x=x))
    assert net._prep[0][-1] == compute and net._prep[1][0].dtype == compute
    rec.done()


# ------------------------------------------------------------------------------------------------ (e) reused workspace
@TYPES
def test_workspace_reused_across_shapes(cuda, td):
    """mid, corner, mid on one module: the second call needs a smaller cell map and reuses the first's memory; the third equals the
    first bit for bit"""
    rec = Recorder(f"bev workspace mid / corner / mid {str(td)[6:]}")
    net = _module(cuda, 2)
    refs = {name: reference(rec, net, name, td) for name in ("mid", "corner")}
    first = run(net, "mid", td, refs["mid"].x, cuda).clone()
    ws = net._ws
    need = lambda name: RB.CASES[name][0] * RB.CASES[name][1][1] * RB.CASES[name][1][2] * 4
    assert ws.numel() == need("mid") > need("corner")
    second = run(net, "corner", td, refs["corner"].x, cuda).clone()
    assert net._ws is ws
    third = run(net, "mid", td, refs["mid"].x, cuda)
    assert net._ws is ws
    check(rec, "mid", first, refs["mid"])
    check(rec, "corner behind mid", second, refs["corner"])
    assert torch.equal(first.view(torch.int32), third.view(torch.int32)), "the third call's map differs from the first's in its bits"
    rec.done()


# ------------------------------------------------------------------------------------------------ (f) the writer alone
@pytest.mark.parametrize("name", ["mid", "solid", "d1-odd"])
def test_dense_writer_with_fill(cuda, name):
    """fnp_sparse_to_dense_fill, f32, C = 128, on the output sites of a case with arbitrary rows and an arbitrary background of both
    signs, into a buffer full of NaN: the numpy scatter bit for bit.  Rows behind n are NaN and name cell 0."""
    idx, B, (D, H, W) = RB.sites(name)
    out = ranked(name)[0]
    n, spare = out.shape[0], 7
    tc = RB.tile_classes(out, B, H, W)
    print(f"\nFORM writer {name} | B {B} plane {H} x {W} | n {n} | tiles of {tc['tile']} cells: {tc['empty']} empty, {tc['slots']} of 1 .. 64, {tc['over']} above 64")
    if name == "mid":
        assert tc["empty"] and tc["slots"] and tc["over"] and tc["partial"] and tc["tile"] == 128
    elif name == "solid":
        assert tc["empty"] == tc["slots"] == 0 and tc["over"] and not tc["partial"] and tc["tile"] == 128
    else:
        assert tc["tile"] == 64 and tc["partial"] and tc["slots"]
    rng = np.random.default_rng(8)
    rows = np.full((n + spare, 128), np.nan, np.float32)
    rows[:n] = rng.standard_normal((n, 128)).astype(np.float32)
    fill = rng.standard_normal(128).astype(np.float32)
    coords = np.zeros((n + spare, 4), np.int32)
    coords[:n] = out
    buf = torch.full((B, 128, 1, H, W), float("nan"), dtype=F32, device=cuda)
    ws = torch.empty((int(_l.load().fnp_sparse_to_dense_workspace_bytes(B, 1, H, W)),), dtype=torch.uint8, device=cuda)
    got = S.to_dense(_dev(rows, cuda), _dev(coords, cuda), S.device_scalar(n, cuda), B, [1, H, W], workspace=ws, out=buf, fill=_dev(fill, cuda))
    assert got.data_ptr() == buf.data_ptr()
    want = RB.scatter(out, rows[:n], fill, B, H, W)
    have = got.view(B, 128, H, W).cpu().numpy()
    bad = np.argwhere((have.view(np.int32) != want.view(np.int32)).any(1))
    assert bad.shape[0] == 0, f"{bad.shape[0]} cells differ from the scatter in their bits, first (b, y, x) {bad[:6].tolist()}; tile of the first: " \
                              f"{(bad[0][1] * W + bad[0][2]) // tc['tile']}"
