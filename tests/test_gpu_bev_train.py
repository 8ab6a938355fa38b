"""The first BaseBEVBackbone block on sparse rows IN TRAINING: csrc/bev_bn.hip (BatchNorm2d with batch statistics over all cells
of the map, ReLU and the dense write, forward and backward) against the float64 reference and DERIVED bounds of
tests/ref_bev_train.py; the (D, 3, 3) rulebook under spconv.conv.SparseConvFunction against tests/ref64.py; and the module with
FNP_SPARSE_FIRST_TRAIN / FNP_DEFER_DENSE.  The site sets are those of ref_bev.CASES (not `full`) plus two scenes of which one has
no row.  The ratios printed are for the record, never a criterion."""
import numpy as np
import pytest
import torch

import ref32 as R32
import ref64 as R
import ref_bev as RB
import ref_bev_train as RT
from findnpropagate_amd import lib as _l
from findnpropagate_amd import sparse as S
from findnpropagate_amd import spconv
from findnpropagate_amd.backbones_2d import BaseBEVBackbone, HeightCompression
from findnpropagate_amd.backbones_2d import bev_norm
from findnpropagate_amd.spconv.conv import SparseConvFunction

pytestmark = pytest.mark.gpu

F32, BF16, FP16 = torch.float32, torch.bfloat16, torch.float16
TYPES = pytest.mark.parametrize("td", [F32, BF16, FP16], ids=["f32", "bf16", "fp16"])
NAMES = ["corner", "d1-odd", "isolated", "solid", "mid", "one-empty"]
C = 128
CFG = {"LAYER_NUMS": [1], "LAYER_STRIDES": [1], "NUM_FILTERS": [128], "UPSAMPLE_STRIDES": [1], "NUM_UPSAMPLE_FILTERS": [32]}


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def sites(name):
    """input sites (n, 4) [b, z, y, x], B, (D, H, W).  one-empty: the sites of `isolated`'s first scene in a batch of two"""
    if name == "one-empty":
        idx, _, shape = RB.sites("isolated")
        return np.ascontiguousarray(idx[idx[:, 0] == 0]), 2, shape
    return RB.sites(name)


_TAB = {}


def table(name):
    if name not in _TAB:
        idx, B, shape = sites(name)
        _TAB[name] = RB.neighbours(idx, B, shape)
    return _TAB[name]


# ------------------------------------------------------------------------------------------------ the operator alone
def _operator(cuda, x, coords, n, B, H, W, gamma, beta, rm, rv, G, td, spare):
    """both calls through the C ABI on stored inputs -> dict of numpy arrays (maps and rows widened to f32)"""
    L = _l.load()
    cap = n + spare
    xr = np.full((cap, C), np.nan, np.float32)
    xr[:n] = x
    cd = np.zeros((cap, 4), np.int32)
    cd[:n] = coords
    xd, cdd, nd = _dev(xr, cuda).to(td), _dev(cd, cuda), S.device_scalar(n, cuda)
    g32, b32, rmd, rvd = (_dev(a, cuda) for a in (gamma, beta, rm, rv))
    nbt = torch.full((1,), 5, dtype=torch.int64, device=cuda)
    y = torch.full((B, C, H, W), float("nan"), dtype=td, device=cuda)
    mean, invstd, fill = (torch.full((C,), float("nan"), dtype=F32, device=cuda) for _ in range(3))
    ws = torch.empty((int(L.fnp_bev_bn_workspace_bytes(C, B, H, W)),), dtype=torch.uint8, device=cuda)
    rc = L.fnp_bev_bn_train_forward(_l.ptr(xd), _l.dtype_code(xd), _l.ptr(cdd), _l.ptr(nd), cap, C, B, H, W, _l.ptr(g32), _l.ptr(b32),
                                    _l.ptr(rmd), _l.ptr(rvd), RT.MOMENTUM, RT.EPS, _l.ptr(y), _l.ptr(mean), _l.ptr(invstd), _l.ptr(fill),
                                    _l.ptr(nbt), _l.ptr(ws), ws.numel(), _l.stream())
    _l.check(rc, "fnp_bev_bn_train_forward")
    Gd = _dev(G, cuda).to(td)
    dx = torch.full((cap, C), float("nan"), dtype=td, device=cuda)
    dgamma, dbeta = (torch.full((C,), float("nan"), dtype=F32, device=cuda) for _ in range(2))
    ws2 = torch.empty_like(ws)
    rc = L.fnp_bev_bn_train_backward(_l.ptr(Gd), _l.ptr(xd), _l.dtype_code(xd), _l.ptr(cdd), _l.ptr(nd), cap, C, B, H, W, _l.ptr(g32),
                                     _l.ptr(b32), _l.ptr(mean), _l.ptr(invstd), _l.ptr(fill), _l.ptr(dx), _l.ptr(dgamma), _l.ptr(dbeta),
                                     _l.ptr(ws2), ws2.numel(), _l.stream())
    _l.check(rc, "fnp_bev_bn_train_backward")
    torch.cuda.synchronize()
    f = lambda t: t.float().cpu().numpy()
    return dict(save_mean=f(mean), save_invstd=f(invstd), fill=f(fill), running_mean=f(rmd), running_var=f(rvd), y=f(y), dx=f(dx),
                dgamma=f(dgamma), dbeta=f(dbeta), nbt=int(nbt.item()))


@TYPES
@pytest.mark.parametrize("name", NAMES)
def test_operator_on_stored_inputs(cuda, name, td):
    _, B, (D, H, W) = sites(name)
    out = table(name)[0]
    n = out.shape[0]
    seed = NAMES.index(name)
    x, gamma, beta, rm, rv = RT.draw_operator(seed, n, C, td)
    G = RT.draw_gradient(seed, B, C, H, W, td)
    st, fwd = RT.reference(x, out, n, B, H, W, gamma, beta, rm, rv, td)
    f64 = fwd["fill"][0].numpy()
    assert RT.gates_exercised(f64), ((f64 > 0).sum(), (f64 == 0).sum())     # (before any device result is looked at)
    got = _operator(cuda, x, out, n, B, H, W, gamma, beta, rm, rv, G, td, spare=5)
    fail, worst = RT.check_forward(got, fwd, out, n, td)
    assert got["nbt"] == 6, got["nbt"]
    # row 0 holds x = 0: the apply's bits for it ARE fill's
    b, _, yy, xx = out[0]
    bg = got["fill"] if td == F32 else torch.from_numpy(got["fill"]).to(td).float().numpy()
    assert np.array_equal(got["y"][b, :, yy, xx].view(np.int32), bg.view(np.int32)), "fill is not the apply's result for x = 0 in its bits"
    fail2, worst2 = RT.check_backward(got, x, G, got["y"], got["fill"], out, n, B, H, W, gamma, td, st)
    worst.update(worst2)
    print(f"\nRATIO bev_bn {name} {str(td)[6:]} n={n} N={B * H * W} | " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert not (fail + fail2), "\n".join(fail + fail2)
    again = _operator(cuda, x, out, n, B, H, W, gamma, beta, rm, rv, G, td, spare=5)
    for k, v in got.items():
        if k != "nbt":
            assert np.array_equal(np.asarray(v).view(np.int32), np.asarray(again[k]).view(np.int32)), f"{k} differs between two runs"


def test_operator_rejects_other_shapes(cuda):
    L = _l.load()
    t = torch.zeros((64, 256), dtype=F32, device=cuda)
    z = torch.zeros((4096,), dtype=F32, device=cuda)
    ws = torch.empty((int(L.fnp_bev_bn_workspace_bytes(256, 1, 8, 8)),), dtype=torch.uint8, device=cuda)
    for Cx, dt in ((24, 0), (256, 0), (4, 0), (128, 7)):
        rc = L.fnp_bev_bn_train_forward(_l.ptr(t), dt, _l.ptr(z), _l.ptr(z), 4, Cx, 1, 8, 8, _l.ptr(z), _l.ptr(z), None, None, 0.01, 1e-3,
                                        _l.ptr(z), _l.ptr(z), _l.ptr(z), _l.ptr(z), None, _l.ptr(ws), ws.numel(), _l.stream())
        assert rc == -1, (Cx, dt, rc)


# ------------------------------------------------------------------------------------------------ SparseConvFunction at (D, 3, 3)
@pytest.mark.parametrize("td", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", NAMES)
def test_strided_rulebook_under_autograd(cuda, name, td):
    """forward, data gradient and weight gradient of the (D, 3, 3) stride-1 table (K = 18 / 9) through SparseConvFunction on the
    permuted view of a Conv2d weight, against ref64.conv / dgrad / wgrad with their bounds"""
    idx, B, shape = sites(name)
    D, H, W = shape
    out, nbr = table(name)
    n_in, m = idx.shape[0], out.shape[0]
    rng = np.random.default_rng(77)
    rd = (lambda a: a) if td == F32 else (lambda a: R.round16(a, td))
    x = rd(rng.standard_normal((n_in, C)).astype(np.float32))
    w2d = rd(RB.stable_weight(rng.uniform(-0.03, 0.03, (C, C * D, 3, 3)).astype(np.float32)))
    dy = rd(rng.standard_normal((m, C)).astype(np.float32))
    wp = RB.weight3d(w2d, D)
    xd = _dev(x, cuda).to(td).requires_grad_(True)
    wd = _dev(w2d, cuda).requires_grad_(True)
    t = spconv.SparseConvTensor(xd, _dev(idx, cuda), list(shape), B)
    n_dev = t.n_dev()
    cap_out = RB.cap_out_of(n_in, B, H, W)
    rb = S.rulebook_strided(t.indices, n_dev, t.rank_grid(), (D, 3, 3), 1, (0, 1, 1), cap_out)
    w3 = wd.view(C, C, D, 3, 3).permute(0, 2, 3, 4, 1)
    rows = SparseConvFunction.apply(xd, w3, rb, rb.out_n, n_dev, False, None, None)
    assert int(rb.out_n.item()) == m and rows.dtype == td and rows.shape == (cap_out, C)
    order = R.match_rows(out, rb.out_indices[:m].cpu().numpy(), [1, H, W])
    dyd = torch.zeros((cap_out, C), dtype=td, device=cuda)
    dyd[:m] = _dev(dy[order], cuda).to(td)
    rows.backward(dyd)
    E = R32.epilogue if td == F32 else (lambda s: R.epilogue(s, out_dtype=td))
    sf, sd, sw = R.conv(x, wp, nbr), R.dgrad(dy, wp, nbr, n_in), R.wgrad(x, dy, nbr)
    o = torch.from_numpy(order)
    Vf, ef = E(sf)
    Vd, ed = E(sd)
    K = D * 9
    if td == F32:
        Vw, ew = sw.S, R32.wgrad_bound(sw, R32.wgrad_partials(min(cap_out, dyd.shape[0]), C, C, K, False)).expand_as(sw.S)
    else:
        Vw, ew = R.epilogue(sw)
    fails, ratios = [], []
    for what, got, V, e in (("forward", rows[:m].detach(), Vf[o], ef[o]), ("dgrad", xd.grad, Vd, ed),
                            ("wgrad", torch.from_numpy(RB.weight3d(wd.grad.float().cpu().numpy(), D)), Vw, ew)):
        worst, rep = R.check(got.float(), V, e)
        ratios.append(f"{what} {worst:.3g}")
        if rep is not None:
            fails.append(f"{what}: {rep}")
    print(f"\nRATIO (D,3,3) autograd {name} {str(td)[6:]} K={K} n_in={n_in} m={m} | " + " ".join(ratios))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ the module
MOD_CASE = "isolated"      # 2 x (2, 40, 40): 2,304-term products, small enough for torch's float64 autograd on the CPU


def _module(cuda, D=2, train=True, **extra):
    rng = np.random.default_rng(4321)
    net = BaseBEVBackbone(dict(CFG, **extra), C * D).to(cuda)
    with torch.no_grad():
        for mod in net.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                k = mod.num_features
                mod.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, k).astype(np.float32)))
                mod.bias.copy_(torch.from_numpy((rng.uniform(0.3, 0.6, k) * np.where(np.arange(k) % 2 == 0, 1, -1)).astype(np.float32)))
                mod.running_mean.copy_(torch.from_numpy(rng.standard_normal(k).astype(np.float32) * 0.2))
                mod.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, k).astype(np.float32)))
        conv = net.blocks[0][1]
        bound = 1.0 / np.sqrt(9.0 * conv.in_channels)
        conv.weight.copy_(torch.from_numpy(RB.stable_weight(rng.uniform(-bound, bound, tuple(conv.weight.shape)).astype(np.float32))))
    return net.train(train)


def _inputs(cuda, name=MOD_CASE):
    idx, B, shape = sites(name)
    x = RB.draw_rows(name if name != "one-empty" else "isolated", F32)[:idx.shape[0]]
    G = np.random.default_rng(99).standard_normal((B, C, shape[1], shape[2])).astype(np.float32)
    return idx, B, shape, x, G


def _tensor(cuda, idx, B, shape, x, dtype=F32):
    feats = _dev(x, cuda).to(dtype).requires_grad_(True)
    return feats, spconv.SparseConvTensor(feats, _dev(idx, cuda), list(shape), B)


def _forward_y(net, data):
    """net(data); -> the output of the first block's ZeroPad2d / Conv2d / BatchNorm2d / ReLU as forward() made it (the input of the
    module behind them), on whichever path forward() took"""
    seen = {}
    h = net.blocks[0][4].register_forward_pre_hook(lambda m, inp: seen.__setitem__("y", inp[0]))
    try:
        net(data)
    finally:
        h.remove()
    return seen["y"]


def _first_block(net, data, G):
    """forward() and the backward of sum(y * G) from the first block's output alone; returns y, d rows, dW, dgamma, dbeta"""
    feats = data["encoded_spconv_tensor"].features
    _zero(net, feats)
    y = _forward_y(net, data)
    (y.float() * G).sum().backward()
    return [y.detach()] + _grads(net, feats)


def _by_hand(net, t, B, shape):
    D, H, W = shape
    conv, bn = net.blocks[0][1], net.blocks[0][2]
    feats = t.features
    if torch.is_autocast_enabled():
        feats = feats.to(torch.get_autocast_gpu_dtype())
    n_dev = t.n_dev()
    rb = S.rulebook_strided(t.indices, n_dev, t.rank_grid(), (D, 3, 3), 1, (0, 1, 1), RB.cap_out_of(feats.shape[0], B, H, W))
    w3 = conv.weight.view(C, C, D, 3, 3).permute(0, 2, 3, 4, 1)
    rows = SparseConvFunction.apply(feats.contiguous(), w3, rb, rb.out_n, n_dev, False, None, None)
    return bev_norm.bev_bn_act(rows, rb.out_indices, rb.out_n, B, H, W, bn)


def _grads(net, feats):
    conv, bn = net.blocks[0][1], net.blocks[0][2]
    return [feats.grad.clone(), conv.weight.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone()]


def _zero(net, feats):
    conv, bn = net.blocks[0][1], net.blocks[0][2]
    for p in (conv.weight, bn.weight, bn.bias, feats):
        p.grad = None


@pytest.mark.parametrize("amp", [False, True], ids=["f32", "autocast-fp16"])
def test_module_equals_the_hand_made_sequence(cuda, amp):
    """(a), (c), (g): forward() with the key on == rulebook -> SparseConvFunction -> bev_bn_act bit for bit (output and the four
    gradients), under autocast the output is fp16, and nothing between entry and the block's output reads the device: torch's sync
    debug mode raises on any synchronising call of torch's (the library's own calls never synchronise: its ABI has no host read)"""
    idx, B, shape, x, G = _inputs(cuda)
    Gd = _dev(G, cuda)
    net, ref = _module(cuda, FNP_SPARSE_FIRST_TRAIN=True), _module(cuda, FNP_SPARSE_FIRST_TRAIN=True)
    with torch.autocast("cuda", dtype=FP16, enabled=amp):
        feats, t = _tensor(cuda, idx, B, shape, x)
        data = {"encoded_spconv_tensor": t}
        assert net.sparse_train_reasons(data) == []
        t.rank_grid(), t.n_dev()
        relu = {}
        h = net.blocks[0][3].register_forward_hook(lambda m, i, o: relu.__setitem__("ran", True))
        torch.cuda.set_sync_debug_mode("error")
        try:
            y = _forward_y(net, data)
        finally:
            torch.cuda.set_sync_debug_mode("default")
            h.remove()
        assert "ran" not in relu, "forward() took the dense path"
        assert y.dtype == (FP16 if amp else F32) and tuple(y.shape) == (B, C, shape[1], shape[2])
        _zero(net, feats)
        (y.float() * Gd).sum().backward()
        got = [y.detach()] + _grads(net, feats)
        feats2, t2 = _tensor(cuda, idx, B, shape, x)
        y2 = _by_hand(ref, t2, B, shape)
        (y2.float() * Gd).sum().backward()
        want = [y2.detach()] + _grads(ref, feats2)
    for what, a, b in zip(("out", "d rows", "dW", "dgamma", "dbeta"), got, want):
        assert a.dtype == b.dtype and torch.equal(a, b), what
    for a, b in zip(net.blocks[0][2].buffers(), ref.blocks[0][2].buffers()):
        assert torch.equal(a, b)
    assert int(net.blocks[0][2].num_batches_tracked.item()) == 1


def test_module_against_the_dense_route(cuda):
    """(b): for each of output, d rows, dW, dgamma, dbeta and the running statistics the norm-wise error against the float64 dense
    route must not exceed 4 x that of torch's dense f32 path (the module with the key off): both sum the same 2,304-term products
    in f32 in different orders"""
    idx, B, shape, x, G = _inputs(cuda)
    Gd = _dev(G, cuda)
    on, off = _module(cuda, FNP_SPARSE_FIRST_TRAIN=True), _module(cuda)
    conv, bn = off.blocks[0][1], off.blocks[0][2]
    f = lambda t: t.detach().float().cpu().numpy()
    ref = RT.dense_route(idx, x, B, shape, f(conv.weight), f(bn.weight), f(bn.bias), f(bn.running_mean), f(bn.running_var), G)
    res = {}
    for key, net in (("sparse", on), ("torch", off)):
        feats, t = _tensor(cuda, idx, B, shape, x)
        data = {"encoded_spconv_tensor": t}
        if key == "torch":
            data = HeightCompression({"NUM_BEV_FEATURES": C * shape[0]})(dict(data, encoded_spconv_tensor_stride=8))
        y, dfe, dW, dga, dbe = _first_block(net, data, Gd)
        assert (key == "sparse") == (not net.sparse_train_reasons(data))
        b = net.blocks[0][2]
        res[key] = dict(y=y, dfeats=dfe, dW=dW, dgamma=dga, dbeta=dbe, running_mean=b.running_mean, running_var=b.running_var)
    bad = []
    for name in ("y", "dfeats", "dW", "dgamma", "dbeta", "running_mean", "running_var"):
        want = ref[name].double()
        err = {k: float((res[k][name].detach().double().cpu() - want).norm() / want.norm()) for k in res}
        print(f"\nNORMWISE {name}: sparse {err['sparse']:.3e} torch {err['torch']:.3e} ratio {err['sparse'] / max(err['torch'], 1e-300):.3g}")
        if not err["sparse"] <= 4 * err["torch"]:
            bad.append((name, err))
    assert not bad, bad


def test_eval_after_a_training_forward_sees_the_new_statistics(cuda):
    """(d): the eval() route's cache is keyed on buffer versions; after one training forward it must fold the NEW running statistics"""
    idx, B, shape, x, G = _inputs(cuda)
    net = _module(cuda, FNP_SPARSE_FIRST_TRAIN=True)
    feats, t = _tensor(cuda, idx, B, shape, x)
    with torch.no_grad():
        net.eval()
        before = net.first_block_from_sparse(spconv.SparseConvTensor(feats.detach(), t.indices, list(shape), B)).clone()
    net.train()
    net({"encoded_spconv_tensor": t})
    net.eval()
    with torch.no_grad():
        te = spconv.SparseConvTensor(feats.detach(), t.indices, list(shape), B)
        after = net.first_block_from_sparse(te)
        dense = HeightCompression({"NUM_BEV_FEATURES": C * shape[0]})({"encoded_spconv_tensor": te, "encoded_spconv_tensor_stride": 8})["spatial_features"]
        want = net.blocks[0][:4](dense)
    assert not torch.equal(before, after)
    assert float((after - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))


def test_deferred_dense_map(cuda):
    """(e): with both keys on the batch_dict has no spatial_features and the encoded rows get the gradients of the route; with
    FNP_DEFER_DENSE alone the backbone densifies by itself and equals the dense path bit for bit"""
    idx, B, shape, x, G = _inputs(cuda)
    Gd = _dev(G, cuda)
    hc = HeightCompression({"NUM_BEV_FEATURES": C * shape[0], "FNP_DEFER_DENSE": True})
    plain = HeightCompression({"NUM_BEV_FEATURES": C * shape[0]})
    outs = []
    for defer in (True, False):
        net = _module(cuda, FNP_SPARSE_FIRST_TRAIN=True)
        feats, t = _tensor(cuda, idx, B, shape, x)
        data = {"encoded_spconv_tensor": t, "encoded_spconv_tensor_stride": 8}
        data = (hc if defer else plain)(data)
        assert ("spatial_features" in data) == (not defer) and data["spatial_features_stride"] == 8
        assert net.sparse_train_reasons(data) == []
        outs.append(_first_block(net, data, Gd))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # the dense path without a map: key off, deferred
    res = []
    for defer in (True, False):
        net = _module(cuda)
        feats, t = _tensor(cuda, idx, B, shape, x)
        data = (hc if defer else plain)({"encoded_spconv_tensor": t, "encoded_spconv_tensor_stride": 8})
        res.append(_first_block(net, data, Gd))
    # (the same torch kernels on the same map: the forward bit for bit; torch's dense weight gradient is not run-to-run
    #  reproducible on this backend, so the gradients are held to 1e-5 of their norm)
    assert torch.equal(res[0][0], res[1][0])
    for a, b in zip(res[0][1:], res[1][1:]):
        assert float((a - b).norm()) <= 1e-5 * float(b.norm())


def test_keys_off_is_the_dense_path(cuda):
    """(f): with the keys off train() is torch's modules on the dense map, bit for bit"""
    idx, B, shape, x, G = _inputs(cuda)
    net = _module(cuda)
    assert net.sparse_first_train is False
    feats, t = _tensor(cuda, idx, B, shape, x)
    data = HeightCompression({"NUM_BEV_FEATURES": C * shape[0]})({"encoded_spconv_tensor": t, "encoded_spconv_tensor_stride": 8})
    assert "FNP_SPARSE_FIRST_TRAIN is off" in net.sparse_train_reasons(data)
    ref = _module(cuda)
    ref.load_state_dict(net.state_dict())        # (the layers behind the first block are torch's random initialisation)
    want = ref.deblocks[0](ref.blocks[0](data["spatial_features"].detach()))
    got = net(data)["spatial_features_2d"]
    assert torch.equal(got, want)
    for a, b in zip(net.state_dict().values(), ref.state_dict().values()):
        assert torch.equal(a, b)
