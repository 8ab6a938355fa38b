"""The backward ROUTES SparseConvFunction chooses in a 16-bit training step, each held to the float64 reference of tests/ref64.py
through the recorder and layer-local checker of tests/train_trace.py:

  (a) one layer per route, through the module (SubMConv3d / SparseConv3d.forward with grad enabled on a hand-built
      SparseConvTensor), bf16 and fp16, on ref64.draw inputs (derived bound) and on small-integer inputs (every A below 2^24:
      dx and dw bit for bit) — each case asserts the route it relies on before it trusts the result, and prints it;
  (b) prepack_weights against pack_weight_train, bit for bit, across the 32-job chunk, and its invalidation by an in-place edit;
  (c) a whole VoxelResBackBone8x training step on a three-cell-thick wavy sheet (every offset of every layer holds pairs for at
      least 20 % of the rows: nothing degenerates to the centre offset, which is its own mirror), all 21 convolutions layer by
      layer, under `FNP_DTYPE: bf16` and under autocast(fp16) with the loss scaled by a fixed 2^12.

No tolerance is chosen here: every bound is ref64's or ref32's derived one plus the widening for subnormal operands
(train_trace's docstring).  The ratios printed are for the record, never a criterion."""
import time

import numpy as np
import pytest
import torch

import ref32 as R32
import ref64 as R
import ref_index
import train_trace as TT
from findnpropagate_amd import sparse as S
from test_gpu_rows128 import _sheet

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
MEMO = {}          # the reference sums of the last 128 -> 128 case: its two routes run the same operands on the same sites


def _dev(a, cuda, td=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return t if td is None else t.to(td)


_SITES = {}


def sheet_sites(H, W, order):
    """a two-cell-thick wavy sheet in one scene of 5 x H x W cells, n no multiple of 16; rows in rank order or shuffled"""
    k = (H, W, order)
    if k not in _SITES:
        rng = np.random.default_rng(4321)
        idx = _sheet(rng, 1, [5, H, W])
        if idx.shape[0] % 16 == 0:
            idx = idx[:-3]
        # (rank order: by (block, bit) of the rank grid — what a grid without a row permutation stands for)
        idx = idx[ref_index.rank_order(idx, 1, [5, H, W])] if order == "rank" else idx[rng.permutation(idx.shape[0])]
        _SITES[k] = np.ascontiguousarray(idx)
    return _SITES[k], 1, [5, H, W]


def sheet3(rng, B, shape, keep=0.8):
    """test_gpu_rows128._sheet with a third plane: a three-cell-thick wavy sheet per scene"""
    D, H, W = shape
    out = []
    for b in range(B):
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        z0 = ((D - 3) * 0.5 * (1 + np.sin(yy / 7.0 + b) * np.cos(xx / 9.0))).astype(np.int64).clip(0, D - 3)
        for dz in (0, 1, 2):
            k = rng.random((H, W)) < keep
            out.append(np.stack([np.full(k.sum(), b), (z0 + dz)[k], yy[k], xx[k]], 1))
    return np.concatenate(out).astype(np.int32)


def _operands(cin, cout, ksize, n_in, n_out, td, exact, seed):
    """x (n_in, cin), w (module layout) and dy (n_out, cout) as f32 arrays: ref64.draw's (the weight NOT rounded: the function
    rounds the f32 parameter) or small integers"""
    rng = np.random.default_rng(seed)
    k = R._triple(ksize)
    if exact:
        z = R.draw_exact(rng, n_in, n_out, cin, cout, td)
        return z["x"], rng.integers(-2, 3, (cout, *k, cin)).astype(np.float32), z["dy"]
    d = R.draw(rng, n_in, n_out, cin, cout, ksize, td)
    return d["x"], (rng.standard_normal((cout, *k, cin)) * 0.05).astype(np.float32), d["dy"]


def _with_spare(a, cap, seed):
    """rows of finite garbage behind the real ones (a stage's tensors are sized by capacity; rows beyond the count are never zeroed)"""
    if cap == a.shape[0]:
        return a
    g = np.random.default_rng(seed).integers(-2, 3, (cap - a.shape[0], a.shape[1])).astype(a.dtype)
    return np.concatenate([a, g])


class Case:
    """one layer through its module under the recorder: forward, backward on a given gradient, host records"""

    def __init__(self, cuda, name, td, conv, idx, B, shape, cap=None, ranked=False, exact=False, x_grad=True, seed=17):
        from findnpropagate_amd import spconv
        self.t0 = time.perf_counter()
        print()
        self.cuda, self.name, self.td, self.conv, self.exact = cuda, name, td, conv.to(cuda), exact
        self.idx, self.B, self.shape, self.ranked, self.x_grad = idx, B, shape, ranked, x_grad
        self.n = idx.shape[0]
        self.cap = cap or self.n
        cin, cout = conv.in_channels, conv.out_channels
        if conv.subm:
            n_out = self.n
        else:
            n_out = R.neighbours_strided(idx, B, shape, conv.kernel_size, conv.stride, conv.padding)[0].shape[0]
        self.n_out = n_out
        x, w, dy = _operands(cin, cout, conv.kernel_size, self.n, n_out, td, exact, seed)
        with torch.no_grad():
            conv.weight.copy_(_dev(w, cuda))
        self.x_host, self.dy_host = _with_spare(x, self.cap, 5), _with_spare(dy, self.cap if conv.subm else n_out, 6)
        self.d_idx = _dev(np.concatenate([idx, np.zeros((self.cap - self.n, 4), np.int32)]), cuda)
        self.n_dev = S.device_scalar(self.n, cuda)
        self.grid = S.build_grid(self.d_idx, self.n_dev, B, shape, keep_order=False) if ranked else None
        self.spconv = spconv

    def tensor(self, x_grad=None):
        x = _dev(self.x_host, self.cuda, self.td).requires_grad_(self.x_grad if x_grad is None else x_grad)
        return x, self.spconv.SparseConvTensor(x, self.d_idx, self.shape, self.B, n_dev=self.n_dev, rank_grid=self.grid)

    def step(self, x_grad=None, gradient=None, through=None):
        """zero the gradients, forward through the module, backward: -> (trace, x, output tensor)"""
        self.conv.weight.grad = None
        x, st = self.tensor(x_grad)
        with TT.Trace(self.conv) as t:
            out = self.conv(st)
            assert out.features.shape == (self.cap if self.conv.subm else self.n_out, self.conv.out_channels) and out.features.dtype == self.td
            g = _dev(self.dy_host, self.cuda, self.td) if gradient is None else gradient
            if through is None:
                t.backward(out.features, g)
            else:
                through(t, out.features, g)
        return t, x, out

    def check(self, t, memo=None):
        results, fails = TT.check_step(f"{self.name} {'exact' if self.exact else 'draw'}", t.host(), exact=self.exact, memo=memo)
        t_ref = sum(r.t_ref for r in results)
        print(f"TIME {self.name} {'exact' if self.exact else 'draw'} | reference {t_ref:.1f} s | whole case {time.perf_counter() - self.t0:.1f} s")
        assert not fails, "\n".join(fails)
        for r in results:
            assert r.min_share > 0.0, "an offset without a pair"
        return results


def _mirror2(conv, td):
    return S.pack_weight(conv.weight, td).flip(0).transpose(1, 2).contiguous()


def _mirror3(conv, td):
    return S.pack_weight(conv.weight, td).transpose(1, 2).contiguous()


def _forward_packs(t):
    return [c["mirror"] for c in t.called("pack_weight_train", "forward")]


# ------------------------------------------------------------------------------------------------ (a) SubM routes
def _subm_conv(C_in, C_out):
    from findnpropagate_amd import spconv
    return spconv.SubMConv3d(C_in, C_out, 3, padding=1, bias=False, indice_key="k")


@pytest.mark.parametrize("exact", [False, True], ids=["draw", "exact"])
@pytest.mark.parametrize("td", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [32, 64])
def test_ranked_subm_data_gradient_on_the_tile_rulebook(cuda, C, td, exact):
    """32 -> 32 and 64 -> 64 on ranked rows: the backward runs conv_forward(grad_out, mirror-2 slabs, ranked=True) -> the
    tile-rulebook kernel"""
    idx, B, shape = sheet_sites(56, 56, "rank")
    c = Case(cuda, f"subm {C}->{C} ranked n={idx.shape[0]} {td}", td, _subm_conv(C, C), idx, B, shape, cap=idx.shape[0] + 300, ranked=True, exact=exact)
    t, x, out = c.step()
    (rec,) = t.records
    rb = rec.rb
    assert rec.ranked and not rec.prepacked and _forward_packs(t) == [2]
    (call,) = t.called("conv_forward", "backward")
    assert not t.called("conv_dgrad")
    assert call["route"] == S.ROUTE_TILED == S.forward_route(rb, 27, C, C, td, td, c.cap, ranked=True)
    assert call["ranked"] and call["rb"] is rb and torch.equal(call["w"], _mirror2(c.conv, td))
    assert rb._tile_rb is not None and C in rb._tile_rb and rb._sorted is None and rb._nbr_t is None and rb._pairs is not None
    print(f"ROUTE {c.name} | forward {t.called('conv_forward', 'forward')[0]['route']} | data gradient conv_forward {call['route']}, mirror-2 slabs")
    c.check(t)
    assert torch.equal(x.grad, rec._dx) and c.conv.weight.grad.shape == c.conv.weight.shape


_SITES_128 = (124, 124)


@pytest.mark.parametrize("route", ["sorted", "plain"])       # (varies fastest: the two routes of one set of operands run back to back)
@pytest.mark.parametrize("exact", [False, True], ids=["draw", "exact"])
@pytest.mark.parametrize("td", DTYPES, ids=IDS)
def test_ranked_128_channel_data_gradient(cuda, route, td, exact):
    """128 -> 128 on ranked rows: at a row capacity of SORT_MIN_ROWS and more forward and data gradient take the class-sorted sweep
    (n ~ 24 000 real rows under a capacity just above the threshold); the same sites under a capacity below it run conv_dgrad on
    the forward's own table with the mirror-2 slabs"""
    C = 128
    idx, B, shape = sheet_sites(*_SITES_128, "rank")
    n = idx.shape[0]
    assert 20000 < n < 28000 and n % 16
    cap = S.SORT_MIN_ROWS + 37 if route == "sorted" else n + 3000
    assert (cap >= S.SORT_MIN_ROWS) == (route == "sorted")
    if route == "sorted":
        # several 16-row blocks in each of the classes the sheet has (rows with neighbours above only, below only, in both planes)
        cls = np.bincount(R32.zclass(R.neighbours_subm(idx, B, shape)), minlength=4)
        assert (cls >= 64).sum() >= 3, cls
    c = Case(cuda, f"subm 128->128 ranked {route} n={n} cap={cap} {td}", td, _subm_conv(C, C), idx, B, shape, cap=cap, ranked=True, exact=exact)
    t, x, out = c.step()
    (rec,) = t.records
    rb = rec.rb
    assert rec.ranked and _forward_packs(t) == [2] and rb._tile_rb is None and rb._nbr_t is None and rb._pairs is not None
    want = S.forward_route(rb, 27, C, C, td, td, cap, ranked=True)
    if route == "sorted":
        (call,) = t.called("conv_forward", "backward")
        assert not t.called("conv_dgrad") and rb._sorted is not None
        assert call["route"] == S.ROUTE_SORTED == want and call["ranked"] and torch.equal(call["w"], _mirror2(c.conv, td))
        assert t.called("conv_forward", "forward")[0]["route"] == S.ROUTE_SORTED
        said = f"conv_forward {call['route']}, mirror-2 slabs"
    else:
        (call,) = t.called("conv_dgrad", "backward")
        assert not t.called("conv_forward", "backward") and rb._sorted is None and want == S.ROUTE_PLAIN
        assert call["pretransposed"] and call["table"] is rb.nbr and torch.equal(call["w"], _mirror2(c.conv, td))
        said = f"conv_dgrad ({want}) on the forward's table, mirror-2 slabs"
    print(f"ROUTE {c.name} | forward {t.called('conv_forward', 'forward')[0]['route']} | data gradient {said}")
    try:
        c.check(t, memo=MEMO)
    finally:
        for k in list(MEMO)[:-1]:          # (keep one set of sums, not one per case of the session)
            del MEMO[k]
    assert torch.equal(x.grad, rec._dx)


@pytest.mark.parametrize("exact", [False, True], ids=["draw", "exact"])
@pytest.mark.parametrize("td", DTYPES, ids=IDS)
def test_unranked_subm_data_gradient_on_the_mirror_form(cuda, td, exact):
    """16 -> 16, rows in random order (stage 1: the voxeliser's order): conv_dgrad with pretransposed=True on the forward's table"""
    idx, B, shape = sheet_sites(56, 56, "random")
    c = Case(cuda, f"subm 16->16 unranked n={idx.shape[0]} {td}", td, _subm_conv(16, 16), idx, B, shape, exact=exact)
    t, x, out = c.step()
    (rec,) = t.records
    rb = rec.rb
    assert not rec.ranked and _forward_packs(t) == [2]
    (call,) = t.called("conv_dgrad", "backward")
    assert not t.called("conv_forward", "backward")
    assert call["pretransposed"] and call["table"] is rb.nbr and torch.equal(call["w"], _mirror2(c.conv, td))
    assert rb._tile_rb is None and rb._sorted is None and rb._nbr_t is None and rb._pairs is not None
    print(f"ROUTE {c.name} | forward {t.called('conv_forward', 'forward')[0]['route']} | data gradient conv_dgrad pretransposed, the forward's table")
    c.check(t)


@pytest.mark.parametrize("exact", [False, True], ids=["draw", "exact"])
@pytest.mark.parametrize("td", DTYPES, ids=IDS)
def test_padded_first_layer(cuda, td, exact):
    """5 -> 16 in a 16-bit dtype: features and weight are zero-padded to 16 channels (pad_channels), the function sees the padded
    operands, and what reaches the module's parameter and the caller's tensor are the slices"""
    idx, B, shape = sheet_sites(56, 56, "random")
    conv = _subm_conv(5, 16)
    assert conv.pad_channels(td) == 11 and conv.pad_channels(torch.float32) == 0
    c = Case(cuda, f"subm 5->16 padded n={idx.shape[0]} {td}", td, conv, idx, B, shape, exact=exact)
    t, x, out = c.step()
    (rec,) = t.records
    assert rec._f.shape[1] == 16 and rec._w.shape[-1] == 16 and not rec._f[:, 5:].any() and not rec._w[..., 5:].any()
    assert not rec.prepacked and _forward_packs(t) == [2]
    (call,) = t.called("conv_dgrad", "backward")
    assert call["pretransposed"] and call["table"] is rec.rb.nbr and call["w"].shape == (27, 16, 16)
    print(f"ROUTE {c.name} | forward {t.called('conv_forward', 'forward')[0]['route']} on 16 -> 16 | data gradient conv_dgrad pretransposed, padded operands")
    c.check(t)
    assert c.conv.weight.grad.shape == c.conv.weight.shape == (16, 3, 3, 3, 5)
    assert x.grad.shape == (c.n, 5) and torch.equal(x.grad, rec._dx[:, :5])


# ------------------------------------------------------------------------------------------------ (a) strided routes
# (Cin, Cout, kernel, stride, padding, row order, sheet H x W: input and output row counts are no multiples of 16)
STRIDED = [(16, 32, 3, 2, 1, "random", (56, 56)), (64, 128, 3, 2, (0, 1, 1), "rank", (56, 56)), (128, 128, (3, 1, 1), (2, 1, 1), 0, "rank", (52, 60))]


@pytest.mark.parametrize("exact", [False, True], ids=["draw", "exact"])
@pytest.mark.parametrize("td", DTYPES, ids=IDS)
@pytest.mark.parametrize("cin,cout,k,s,p,order,hw", STRIDED, ids=["16-32", "64-128", "conv_out"])
def test_strided_data_gradient_on_the_transposed_table(cuda, cin, cout, k, s, p, order, hw, td, exact):
    """the strided layers as the backbone feeds them: the module takes `rows=` (the output has exactly n_out rows), the forward's
    launch writes the mirror-3 slabs and the data gradient runs on rb._nbr_t.  16 -> 32 then runs a second backward on the same
    rulebook with another input capacity: transposed_table must remake the table."""
    from findnpropagate_amd import spconv
    from findnpropagate_amd.spconv import conv as C
    idx, B, shape = sheet_sites(*hw, order)
    conv = spconv.SparseConv3d(cin, cout, k, stride=s, padding=p, bias=False)
    c = Case(cuda, f"strided {cin}->{cout} k={k} n_in={idx.shape[0]} {td}", td, conv, idx, B, shape, ranked=order == "rank", exact=exact)
    t, x, out = c.step()
    (rec,) = t.records
    rb = rec.rb
    assert rec.rows == c.n_out == out.features.shape[0] and c.n % 16 and c.n_out % 16 and rb.cap_out > c.n_out and _forward_packs(t) == [3]
    (call,) = t.called("conv_dgrad", "backward")
    (made,) = t.called("transposed_table", "backward")
    assert not t.called("conv_forward", "backward")
    assert call["pretransposed"] and call["table"] is rb._nbr_t and rb._nbr_t.shape == (rb.K, c.n) and made["remade"]
    assert torch.equal(call["w"], _mirror3(c.conv, td))
    assert rb._pairs is not None and rb._pairs[0].shape[1] == c.n_out and rb._tile_rb is None and rb._sorted is None
    print(f"ROUTE {c.name} | forward {t.called('conv_forward', 'forward')[0]['route']} rows={rec.rows} | data gradient conv_dgrad on the transposed table, mirror-3 slabs")
    c.check(t)
    if (cin, cout) != (16, 32):
        return
    # the same rulebook (its pair lists and its transposed table are kept with it) under another input capacity
    first, spare = rb._nbr_t, 41
    c.conv.weight.grad = None
    x2 = _dev(_with_spare(c.x_host, c.n + spare, 9), cuda, td).requires_grad_(True)
    with TT.Trace() as t2:
        o2 = C.SparseConvFunction.apply(x2, c.conv.weight, rb, rb.out_n, c.n_dev, False, c.n_out, None)
        t2.backward(o2, _dev(c.dy_host, cuda, td))
    (rec2,) = t2.records
    (made2,) = t2.called("transposed_table", "backward")
    assert made2["remade"] and rb._nbr_t is not first and rb._nbr_t.shape == (rb.K, c.n + spare)
    rec2.adopt(rec)
    c.name += " (second capacity)"
    c.check(t2)
    assert torch.equal(rec2._out, rec._out) and torch.equal(rec2._dx[:c.n], rec._dx) and torch.equal(rec2._dw, rec._dw)


# ------------------------------------------------------------------------------------------------ (a) the autograd contract
@pytest.mark.parametrize("td", DTYPES, ids=IDS)
def test_autograd_contract_of_the_function(cuda, td):
    """32 -> 32 on ranked rows: what the function owes autograd whatever route it takes"""
    from findnpropagate_amd.spconv import conv as C
    Cn = 32
    idx, B, shape = sheet_sites(56, 56, "rank")
    c = Case(cuda, f"contract 32->32 {td}", td, _subm_conv(Cn, Cn), idx, B, shape, ranked=True)
    t, x, out = c.step()
    (base,) = t.records
    c.check(t)
    o0, dx0, dw0 = base._out.clone(), base._dx.clone(), c.conv.weight.grad.clone()

    # two runs: the same bits
    t, x, out = c.step()
    assert torch.equal(t.records[0]._out, o0) and torch.equal(x.grad, dx0) and torch.equal(c.conv.weight.grad, dw0)

    # weight frozen: no weight gradient, the data gradient unchanged
    c.conv.weight.requires_grad_(False)
    try:
        t, x, out = c.step()
    finally:
        c.conv.weight.requires_grad_(True)
    assert c.conv.weight.grad is None and t.records[0]._dw is None and torch.equal(x.grad, dx0)

    # input without grad: no mirror slabs are written, no data gradient is computed, the weight gradient unchanged
    t, x, out = c.step(x_grad=False)
    assert _forward_packs(t) == [0] and x.grad is None and t.records[0]._dx is None
    assert not t.called("conv_forward", "backward") and not t.called("conv_dgrad")
    assert torch.equal(t.records[0]._out, o0) and torch.equal(c.conv.weight.grad, dw0)

    # a non-contiguous gradient (the transpose of a (C, n) tensor)
    t, x, out = c.step(through=lambda t, f, g: t.backward(f.t(), g.t().contiguous()))
    (rec,) = t.host()
    assert rec.go_contiguous is False and torch.equal(x.grad, dx0) and torch.equal(c.conv.weight.grad, dw0)

    # an f32 gradient into 16-bit features: the bits of the gradient rounded beforehand
    g32 = _dev(np.random.default_rng(3).standard_normal((c.cap, Cn)).astype(np.float32), cuda)
    assert not torch.equal(g32.to(td).float(), g32)
    t, x, out = c.step(gradient=g32)
    dx_a, dw_a = x.grad.clone(), c.conv.weight.grad.clone()
    t, x, out = c.step(gradient=g32.to(td))
    assert torch.equal(x.grad, dx_a) and torch.equal(c.conv.weight.grad, dw_a)

    # prepacked slabs of another dtype, or of another mirror mode, are ignored (they hold NaN here); matching ones are used
    rb, g = base.rb, _dev(c.dy_host, cuda, td)
    other = torch.float16 if td == torch.bfloat16 else torch.bfloat16
    nan = lambda dt: torch.full((27, Cn, Cn), float("nan"), dtype=dt, device=cuda)
    good = S.pack_weight_train(c.conv.weight, td, 2)
    for tag, pre, packs in (("another dtype", (other, 2, nan(other), nan(other)), [2]), ("another mirror mode", (td, 3, nan(td), nan(td)), [2]),
                            ("matching", (td, 2) + tuple(good), [])):
        c.conv.weight.grad = None
        x, _ = c.tensor()
        with TT.Trace() as t:
            o = C.SparseConvFunction.apply(x, c.conv.weight, rb, c.n_dev, c.n_dev, True, None, pre)
            t.backward(o, g)
        assert t.records[0].prepacked and _forward_packs(t) == packs, tag
        assert torch.equal(o.detach(), o0) and torch.equal(x.grad, dx0) and torch.equal(c.conv.weight.grad, dw0), tag


# ------------------------------------------------------------------------------------------------ (b) prepack
def _assert_prepacked_bits(m, td):
    pre = m.__dict__.get("_fnp_prepack")
    if m.pad_channels(td):
        assert pre is None          # (its forward pads and packs the padded weight itself)
        return 0
    mode = 2 if (m.subm and all(k & 1 for k in m.kernel_size)) else 3
    assert pre is not None and pre[0] == m.weight._version and pre[1] == m.weight.data_ptr() and pre[2] == td and pre[3] == mode
    p, mm = S.pack_weight_train(m.weight, td, mode)
    assert pre[4].dtype == td and torch.equal(pre[4], p) and torch.equal(pre[5], mm)
    # ... which are the torch ops' bits (test_pack_weight_kernel_equals_the_torch_ops), restated here for the multi-layer launch
    ref = S.pack_weight(m.weight, td)
    assert torch.equal(pre[4], ref) and torch.equal(pre[5], ref.flip(0).transpose(1, 2).contiguous() if mode == 2 else ref.transpose(1, 2).contiguous())
    return 1


@pytest.mark.parametrize("td", [torch.float32] + DTYPES, ids=["f32"] + IDS)
def test_prepack_leaves_the_bits_of_pack_weight_train(cuda, td):
    """prepack_weights (pack_weights_train -> fnp_pack_weight_multi: one launch for all layers, in chunks of 32) writes the slabs
    every layer's forward and data gradient read in a real step: on every layer of VoxelResBackBone8x, and on 33 modules"""
    from findnpropagate_amd import spconv, synthetic as syn
    from findnpropagate_amd.backbones_3d import VoxelResBackBone8x
    from findnpropagate_amd.spconv import conv as C
    net = syn.init_backbone_weights(VoxelResBackBone8x({"USE_BIAS": False, "FNP_DTYPE": "bf16"}, 5, np.array([96, 88, 40])), 0).to(cuda)
    convs = [m for m in net.modules() if isinstance(m, spconv.SparseConvolution)]
    assert len(convs) == 21
    C.prepack_weights([(m, td) for m in convs])
    assert sum(_assert_prepacked_bits(m, td) for m in convs) == (21 if td == torch.float32 else 20)
    C.end_of_backbone_forward(convs)
    assert not any("_fnp_prepack" in m.__dict__ for m in convs)
    shapes = [lambda: spconv.SubMConv3d(16, 16, 3, bias=False), lambda: spconv.SparseConv3d(16, 32, 3, stride=2, padding=1, bias=False),
              lambda: spconv.SparseConv3d(32, 16, (3, 1, 1), stride=(2, 1, 1), bias=False), lambda: spconv.SubMConv3d(32, 32, (1, 3, 3), bias=False)]
    many = [shapes[i % 4]().to(cuda) for i in range(33)]
    C.prepack_weights([(m, td) for m in many])
    assert sum(_assert_prepacked_bits(m, td) for m in many) == 33


@pytest.mark.parametrize("td", DTYPES, ids=IDS)
def test_prepack_is_dropped_when_the_weight_is_edited_in_place(cuda, td):
    """a module's next forward uses its prepacked slabs while the weight is the one they were made of, and repacks after an
    in-place edit: the output is the NEW weight's (a stale prepack is `out` from a weight one update older)"""
    from findnpropagate_amd.spconv import conv as C
    idx, B, shape = sheet_sites(56, 56, "rank")
    c = Case(cuda, f"prepack 32->32 {td}", td, _subm_conv(32, 32), idx, B, shape, ranked=True)
    C.prepack_weights([(c.conv, td)])
    t, x, out = c.step()
    assert t.records[0].prepacked and _forward_packs(t) == []
    c.check(t)
    old = t.records[0]._out.clone()
    with torch.no_grad():
        c.conv.weight.add_(1e-3 * torch.sign(c.conv.weight))          # an optimizer's step
    assert c.conv.__dict__["_fnp_prepack"][0] != c.conv.weight._version
    t, x, out = c.step()
    assert not t.records[0].prepacked and _forward_packs(t) == [2] and not torch.equal(t.records[0]._out, old)
    c.name += " after the edit"
    c.check(t)
    C.end_of_backbone_forward([c.conv])


# ------------------------------------------------------------------------------------------------ (c) the whole step
_STEP_SITES = {}


def step_sites():
    """two scenes of a three-cell-thick wavy sheet on the backbone's grid [96, 88, 40] (sparse shape 41 x 88 x 96), rows shuffled"""
    if not _STEP_SITES:
        rng = np.random.default_rng(2024)
        idx = sheet3(rng, 2, [41, 88, 96])
        _STEP_SITES["idx"] = np.ascontiguousarray(idx[rng.permutation(idx.shape[0])])
        _STEP_SITES["x"] = rng.standard_normal((idx.shape[0], 5)).astype(np.float32)
    return _STEP_SITES["idx"], _STEP_SITES["x"]


@pytest.mark.parametrize("mode", ["bf16", "amp-fp16"])
def test_backbone_step_layer_by_layer(cuda, mode):
    """VoxelResBackBone8x.train(), one step under the recorder with the strided rulebooks prefetched: all 21 convolutions against
    check_layer.  bf16: `FNP_DTYPE: bf16` without autocast (conv_input runs in f32: ref32's bound); amp-fp16: autocast(fp16), the
    loss times a fixed 2^12, no GradScaler (conv_input zero-padded 5 -> 16; the gradients hold fp16 subnormals)."""
    from findnpropagate_amd import spconv, synthetic as syn
    from findnpropagate_amd.backbones_3d import VoxelResBackBone8x
    from findnpropagate_amd.spconv import conv as C
    t0 = time.perf_counter()
    amp = mode == "amp-fp16"
    td = torch.float16 if amp else torch.bfloat16
    grid = np.array([96, 88, 40])
    net = syn.init_backbone_weights(VoxelResBackBone8x({"USE_BIAS": False, "FNP_DTYPE": "fp16" if amp else "bf16"}, 5, grid), 0).to(cuda).train()
    idx, feats = step_sites()
    assert idx.shape[0] > 35000
    bd = {"voxel_features": _dev(feats, cuda), "voxel_coords": _dev(idx, cuda).float(), "batch_size": 2}
    loss_of = lambda out: sum((t.features.float() ** 2).mean() for t in list(out["multi_scale_3d_features"].values()) + [out["encoded_spconv_tensor"]])
    assert C.PREFETCH
    net.zero_grad()
    with TT.Trace(net) as t:
        if amp:
            with torch.autocast("cuda", dtype=torch.float16):
                loss = loss_of(net(bd)) * 2.0 ** 12
        else:
            loss = loss_of(net(bd))
        t.backward(loss)
    assert torch.isfinite(loss)
    recs = t.host()
    assert len(recs) == 21 and len({id(r.module) for r in recs}) == 21
    assert [r.name for r in recs][:5] == ["conv_input.0", "conv1.0.conv1", "conv1.0.conv2", "conv1.1.conv1", "conv1.1.conv2"]
    print(f"\nSITES {mode} | {idx.shape[0]} voxels | strided outputs {[r.n_out for r in recs if not r.subm]}")

    # what the step is meant to exercise, asserted before its results are trusted
    first = recs[0]
    if amp:
        assert first.dtype == td and first.x.shape[1] == 16 and not first.prepacked and first.dw.shape[-1] == 5
    else:
        assert first.dtype == torch.float32 and first.x.shape[1] == 5 and first.prepacked and first.go_dtype == torch.float32
    assert all(r.prepacked and r.dtype == td for r in recs[1:]) and first.dx is None and all(r.dx is not None for r in recs[1:])
    strided = [i for i, r in enumerate(recs) if not r.subm]
    assert strided == [5, 10, 15, 20] and all(recs[i].rows == recs[i].n_out for i in strided)
    assert all(r.ranked == (i > 5) for i, r in enumerate(recs) if r.subm)
    tiled = t.called("conv_forward", "backward")
    assert sorted(c["w"].shape[1] for c in tiled) == [32] * 4 + [64] * 4 and all(c["route"] == S.ROUTE_TILED and c["ranked"] for c in tiled)
    assert len(t.called("conv_dgrad", "backward")) == 12 and all(c["pretransposed"] for c in t.called("conv_dgrad"))
    assert not t.called("pack_weight_train") or (amp and _forward_packs(t) == [0])       # (only the padded layer packs for itself)
    for r in recs:          # one rulebook per stage: its pair lists (and a strided layer's transposed table) are shared, made once
        assert r.rb._pairs is not None and (r.subm or r.rb._nbr_t is not None)
    assert len({id(r.rb) for r in recs}) == 9

    results, fails = TT.check_step(f"step {mode}", recs)
    worst = {}
    for rec, r in zip(recs, results):
        assert r.min_share >= 0.2, (r.name, r.min_share)        # no layer degenerates to the centre offset
        label = f"{'subm' if rec.subm else 'strided'} {rec.x.shape[1]}->{rec.w.shape[0]}{' f32' if rec.dtype == torch.float32 else ''}"
        for q, v in r.ratio.items():
            worst[label, q] = max(worst.get((label, q), 0.0), v)
    for label in dict.fromkeys(k[0] for k in worst):
        print(f"WORST step {mode} | {label} | " + " / ".join(f"{q} {worst[label, q]:.4g}" for q in ("out", "dx", "dw") if (label, q) in worst))
    print(f"SHARE step {mode} | smallest share of rows with a pair, over all offsets and layers: {min(r.min_share for r in results):.3f}")
    print(f"TIME step {mode} | reference {sum(r.t_ref for r in results):.1f} s | whole case {time.perf_counter() - t0:.1f} s")
    assert not fails, "\n".join(fails)
    print(f"SUBNORMAL step {mode} | largest share of subnormal gradient operands in a layer {max(r.sub['go'] for r in results):.3g}")
