"""Backward of SparseConvTensor.dense() / HeightCompression (fnp_sparse_to_dense_backward, sparse.DenseFunction) and the fp16
densify, on the MI355X.  The reference's spconv builds the dense map with a torch index assignment (out[b, :, z, y, x] = features),
so torch autograd of `torch.zeros(...).index_put((b, z, y, x), features)` is the yardstick: the adjoint is a copy, so every
comparison with it is bit for bit."""
import gc

import numpy as np
import pytest
import torch

from findnpropagate_amd import lib as _l, sparse as S, spconv

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _sites(rng, B, D, H, W, kind, frac=0.1):
    """unique (b, z, y, x) int32 rows in random order.  clustered: blobs of ~frac of the cells; rows: whole lines y of plane 0
    filled (tiles with more rows than LDS slots) plus a sprinkle; empty_scene: scene 1 holds nothing."""
    cells = B * D * H * W
    if kind == "clustered":
        m = np.zeros((B, D, H, W), bool)
        for b in range(B):
            cy, cx = rng.integers(0, H, 12), rng.integers(0, W, 12)
            k = rng.integers(0, 12, int(frac * D * H * W) + 1)
            y = np.clip(cy[k] + rng.normal(0, H / 12, k.shape), 0, H - 1).astype(int)
            x = np.clip(cx[k] + rng.normal(0, W / 12, k.shape), 0, W - 1).astype(int)
            m[b, rng.integers(0, D, k.shape), y, x] = True
        lin = np.flatnonzero(m.ravel())
    elif kind == "rows":
        m = np.zeros((B, D, H, W), bool)
        m[:, 0, 1:4, :] = True
        m.ravel()[rng.choice(cells, size=cells // 20, replace=False)] = True
        lin = np.flatnonzero(m.ravel())
    else:
        lin = rng.choice(cells, size=max(1, int(frac * cells)), replace=False)
        if kind == "empty_scene":
            lin = lin[lin // (D * H * W) != 1]
    lin = lin[rng.permutation(lin.shape[0])]
    b, rem = np.divmod(lin, D * H * W)
    z, rem = np.divmod(rem, H * W)
    y, x = np.divmod(rem, W)
    return np.stack([b, z, y, x], 1).astype(np.int32)


def _torch_dense(f, idx, B, shape):
    """the reference's dense(): zeros + index assignment (rows in the grid only), channels first"""
    C = f.shape[1]
    i = idx.long()
    d = torch.zeros((B, *shape, C), dtype=f.dtype, device=f.device).index_put((i[:, 0], i[:, 1], i[:, 2], i[:, 3]), f)
    return d.permute(0, 4, 1, 2, 3)


CASES = {   # (B, C, (D, H, W), sites)
    "shipped": (2, 128, (2, 180, 180), "clustered"),
    "odd_plane": (3, 16, (3, 7, 9), "random"),
    "c5": (2, 5, (2, 12, 16), "random"),
    "overflow": (2, 32, (2, 8, 256), "rows"),
    "empty_scene": (3, 64, (2, 20, 24), "empty_scene"),
}


@pytest.mark.parametrize("dtype", ["f32", "bf16", "fp16"])
@pytest.mark.parametrize("case", list(CASES) + ["n0"])
def test_adjoint_equals_torch_index_put(cuda, rng, dtype, case):
    B, C, shape, kind = CASES["odd_plane" if case == "n0" else case]
    idx = _sites(rng, B, *shape, kind)
    td = DT[dtype]
    f = torch.from_numpy(rng.standard_normal((idx.shape[0], C)).astype(np.float32)).to(cuda).to(td).requires_grad_(True)
    di = torch.from_numpy(idx).to(cuda)
    n = 0 if case == "n0" else idx.shape[0]
    G = torch.from_numpy(rng.standard_normal((B, C, *shape)).astype(np.float32)).to(cuda).to(td)
    out = S.to_dense(f, di, S.device_scalar(n, cuda), B, list(shape))
    assert out.grad_fn is not None and out.dtype == td
    got, = torch.autograd.grad(out, f, G)
    f2 = f.detach().clone().requires_grad_(True)
    ref = _torch_dense(f2[:n], di[:n], B, shape)
    assert torch.equal(out.detach(), ref.detach())
    want, = torch.autograd.grad(ref, f2, G, allow_unused=True)
    if want is None:
        want = torch.zeros_like(f2)
    assert got.dtype == td and got.shape == f.shape
    assert torch.equal(got, want)
    got2, = torch.autograd.grad(S.to_dense(f, di, S.device_scalar(n, cuda), B, list(shape)), f, G)
    assert torch.equal(got, got2), "two backwards differ"


def _raw_backward(G, idx, n, cap, B, shape, workspace=True, prefill=7.0):
    """fnp_sparse_to_dense_backward into a buffer that holds `prefill` everywhere: every row must be written"""
    L = _l.load()
    C = G.shape[1]
    gf = torch.full((cap, C), prefill, dtype=G.dtype, device=G.device)
    ws = torch.empty((int(L.fnp_sparse_to_dense_workspace_bytes(B, *shape)),), dtype=torch.uint8, device=G.device) if workspace else None
    n_dev = S.device_scalar(n, G.device)
    rc = L.fnp_sparse_to_dense_backward(_l.ptr(G), _l.dtype_code(G), _l.ptr(idx), _l.ptr(n_dev), cap, C, B, *shape, _l.ptr(gf),
                                        _l.ptr(ws), 0 if ws is None else ws.numel(), _l.stream())
    _l.check(rc, "fnp_sparse_to_dense_backward")
    return gf


@pytest.mark.parametrize("dtype,C,workspace", [("f32", 128, True), ("bf16", 128, True), ("fp16", 64, True), ("fp16", 5, True),
                                               ("bf16", 128, False), ("f32", 3, False)])
def test_padded_and_out_of_grid_rows_get_zero(cuda, rng, dtype, C, workspace):
    B, shape = 2, (2, 24, 40)
    idx = _sites(rng, B, *shape, "random", frac=0.15)
    cap = idx.shape[0]
    n = cap - 37                          # rows n .. cap-1: padding (their coordinates are in the grid: still 0)
    bad = rng.choice(n, size=25, replace=False)
    lim = np.array([B, *shape])
    for k, r in enumerate(bad):           # out-of-grid rows among the first n: negative or past the end on every axis in turn
        ax = k % 4
        idx[r, ax] = -1 - k if k % 2 else lim[ax] + k
    G = torch.from_numpy(rng.standard_normal((B, C, *shape)).astype(np.float32)).to(cuda).to(DT[dtype])
    got = _raw_backward(G, torch.from_numpy(idx).to(cuda), n, cap, B, shape, workspace=workspace)
    g = G.cpu()
    want = torch.zeros((cap, C), dtype=G.dtype)
    for r in range(n):
        b, z, y, x = (int(v) for v in idx[r])
        if 0 <= b < B and 0 <= z < shape[0] and 0 <= y < shape[1] and 0 <= x < shape[2]:
            want[r] = g[b, :, z, y, x]
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("C", [128, 6])
@pytest.mark.parametrize("with_fill", [False, True])
def test_fp16_forward_equals_index_put(cuda, rng, C, with_fill):
    B, shape = 2, (2, 36, 40)
    idx = torch.from_numpy(_sites(rng, B, *shape, "clustered")).to(cuda)
    f = torch.from_numpy(rng.standard_normal((idx.shape[0], C)).astype(np.float32)).to(cuda).half()
    fill = torch.from_numpy(rng.standard_normal(C).astype(np.float32)).to(cuda) if with_fill else None
    got = S.to_dense(f, idx, S.device_scalar(idx.shape[0], cuda), B, list(shape), fill=fill)
    want = _torch_dense(f, idx, B, shape).contiguous()
    if with_fill:
        bg = torch.zeros((B, *shape, C), dtype=torch.bool, device=cuda)
        i = idx.long()
        bg[i[:, 0], i[:, 1], i[:, 2], i[:, 3]] = True
        want = torch.where(bg.permute(0, 4, 1, 2, 3), want, fill.half().view(1, C, 1, 1, 1))
    assert got.dtype == torch.float16 and torch.equal(got, want)


def _tensor(rng, cuda, B, shape, C, dtype=torch.float32, frac=0.1):
    idx = _sites(rng, B, *shape, "clustered", frac)
    f = torch.from_numpy(rng.standard_normal((idx.shape[0], C)).astype(np.float32)).to(cuda).to(dtype).requires_grad_(True)
    return f, spconv.SparseConvTensor(f, torch.from_numpy(idx).to(cuda), list(shape), B)


@pytest.mark.parametrize("channels_first", [True, False])
def test_sparse_conv_tensor_dense_gradient(cuda, rng, channels_first):
    B, shape, C = 2, (2, 30, 36), 32
    f, t = _tensor(rng, cuda, B, shape, C)
    d = t.dense(channels_first=channels_first)
    ref = _torch_dense(f, t.indices, B, shape)
    if not channels_first:
        ref = ref.permute(0, 2, 3, 4, 1)
    assert torch.equal(d.detach(), ref.detach())
    G = torch.randn(d.shape, device=cuda)
    got, = torch.autograd.grad(d, f, G)
    want, = torch.autograd.grad(ref, f, G)
    assert torch.equal(got, want)


def test_height_compression_is_on_the_graph_with_its_cast(cuda, rng):
    from findnpropagate_amd.backbones_2d import HeightCompression
    B, shape, C = 2, (2, 30, 36), 64
    f, t = _tensor(rng, cuda, B, shape, C)
    hc = HeightCompression({"NUM_BEV_FEATURES": C * 2, "OUT_DTYPE": "bf16"})
    sf = hc({"encoded_spconv_tensor": t, "encoded_spconv_tensor_stride": 8})["spatial_features"]
    assert sf.requires_grad and sf.dtype == torch.bfloat16 and tuple(sf.shape) == (B, C * 2, 30, 36)
    G = torch.randn(sf.shape, device=cuda)
    (sf.float() * G).sum().backward()
    f2 = f.detach().clone().requires_grad_(True)
    ref = _torch_dense(f2.to(torch.bfloat16), t.indices, B, shape).reshape(B, C * 2, 30, 36)
    (ref.float() * G).sum().backward()
    assert f.grad.dtype == torch.float32 and torch.equal(f.grad, f2.grad)
    assert float(f.grad.abs().max()) > 0


def _two_forwards_two_backwards(cuda, rng_seed, reuse):
    from findnpropagate_amd.backbones_2d import HeightCompression
    rng = np.random.default_rng(rng_seed)
    B, shape, C = 2, (2, 20, 24), 16
    hc = HeightCompression({"NUM_BEV_FEATURES": C * 2, "REUSE_OUTPUT": reuse})
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(C * 2, 8, 3, padding=1, bias=False).to(cuda)
    fs, ys = [], []
    for _ in range(2):                    # gradient accumulation over two micro-batches: both forwards before any backward
        f, t = _tensor(rng, cuda, B, shape, C)
        fs.append(f)
        ys.append(conv(hc({"encoded_spconv_tensor": t, "encoded_spconv_tensor_stride": 8})["spatial_features"]))
    for y in ys:
        (y ** 2).sum().backward()
    return conv.weight.grad.clone(), [f.grad.clone() for f in fs]


def test_reused_output_is_not_shared_by_graphs(cuda):
    w0, g0 = _two_forwards_two_backwards(cuda, 5, False)
    w1, g1 = _two_forwards_two_backwards(cuda, 5, True)
    assert torch.allclose(w1, w0, rtol=1e-5, atol=1e-5), float((w1 - w0).abs().max())
    for a, b in zip(g1, g0):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5)


def test_no_grad_keeps_the_reused_buffer(cuda, rng):
    from findnpropagate_amd.backbones_2d import HeightCompression
    B, shape, C = 2, (2, 20, 24), 16
    hc = HeightCompression({"NUM_BEV_FEATURES": C * 2, "REUSE_OUTPUT": True})
    f, t = _tensor(rng, cuda, B, shape, C)
    bd = lambda: {"encoded_spconv_tensor": t, "encoded_spconv_tensor_stride": 8}
    with torch.no_grad():
        a = hc(bd())["spatial_features"]
        buf = hc._out
        b = hc(bd())["spatial_features"]
    assert a.grad_fn is None and b.grad_fn is None and hc._out is buf and b.data_ptr() == a.data_ptr()
    c = hc(bd())["spatial_features"]      # grad on: a fresh tensor, the buffer stays the no-grad one
    assert c.grad_fn is not None and c.data_ptr() != buf.data_ptr() and hc._out is buf
    # fill form (BaseBEVBackbone's eval-only sparse first block): never differentiable
    fill = torch.zeros(C, device=cuda)
    assert S.to_dense(f, t.indices, t.n_dev(), B, list(shape), fill=fill).grad_fn is None


BEV_CFG = {"LAYER_NUMS": [1, 1], "LAYER_STRIDES": [1, 1], "NUM_FILTERS": [64, 64], "UPSAMPLE_STRIDES": [1, 1],
           "NUM_UPSAMPLE_FILTERS": [64, 64], "USE_CONV_FOR_NO_STRIDE": True}


@pytest.mark.parametrize("amp", [False, True])
def test_detector_loss_reaches_the_3d_backbone(cuda, amp):
    """VoxelResBackBone8x (train) -> HeightCompression -> BaseBEVBackbone (train), loss on spatial_features_2d: every backbone
    parameter gets a gradient, the encoded rows get spatial_features.grad at their cells, and seeding the backbone's own
    backward with those rows gives the same parameter gradients bit for bit."""
    from findnpropagate_amd import synthetic as syn
    from findnpropagate_amd.backbones_2d import BaseBEVBackbone, HeightCompression
    from findnpropagate_amd.backbones_3d import VoxelResBackBone8x
    rng = np.random.default_rng(77)
    grid = np.array([96, 88, 40])
    cfg = {"USE_BIAS": False, "FNP_DTYPE": "fp32"}
    if amp:
        cfg["FNP_OUT_DTYPE"] = "native"
    net = syn.init_backbone_weights(VoxelResBackBone8x(cfg, 5, grid), 0).to(cuda).train()
    D3, H3, W3 = net.sparse_shape
    cells = 2 * D3 * H3 * W3
    lin = rng.choice(cells, size=5000, replace=False)
    b, rem = np.divmod(lin, D3 * H3 * W3); z, rem = np.divmod(rem, H3 * W3); y, x = np.divmod(rem, W3)
    feats = rng.standard_normal((5000, 5)).astype(np.float32)
    coords = np.stack([b, z, y, x], 1).astype(np.int32)
    bd = lambda: {"voxel_features": torch.from_numpy(feats).to(cuda), "voxel_coords": torch.from_numpy(coords).to(cuda).float(), "batch_size": 2}
    hc = HeightCompression({"NUM_BEV_FEATURES": 256})
    bev = BaseBEVBackbone(BEV_CFG, 256).to(cuda).train()
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 8) if amp else None

    net.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        out = net(bd())
        enc = out["encoded_spconv_tensor"]
        enc.features.retain_grad()
        d = hc(dict(out))
        d["spatial_features"].retain_grad()
        loss = (bev(d)["spatial_features_2d"].float() ** 2).mean()
    assert enc.features.dtype == (torch.float16 if amp else torch.float32)
    (scaler.scale(loss) if amp else loss).backward()
    grads = {k: p.grad for k, p in net.named_parameters()}
    for k, g in grads.items():
        assert g is not None, k
        assert bool(torch.isfinite(g).all()), k
        assert float(g.abs().max()) > 0, k

    sg = d["spatial_features"].grad
    C = enc.features.shape[1]
    n = int(enc.n_dev().item())
    i = enc.indices[:n].long()
    gathered = torch.zeros_like(enc.features)
    gathered[:n] = sg.view(2, C, *enc.spatial_shape).permute(0, 2, 3, 4, 1)[i[:, 0], i[:, 1], i[:, 2], i[:, 3]]
    assert enc.features.grad.dtype == sg.dtype == gathered.dtype
    assert torch.equal(enc.features.grad, gathered)

    grads = {k: g.clone() for k, g in grads.items()}
    net.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        out2 = net(bd())
    torch.autograd.backward(out2["encoded_spconv_tensor"].features, gathered)
    for k, p in net.named_parameters():
        assert torch.equal(p.grad, grads[k]), (k, float((p.grad - grads[k]).abs().max()))


def test_captured_forward_backward_replays_the_eager_result(cuda, rng):
    B, shape, C = 2, (2, 64, 72), 128
    idx = torch.from_numpy(_sites(rng, B, *shape, "clustered")).to(cuda)
    n_dev = S.device_scalar(idx.shape[0], cuda)
    L = _l.load()
    ws = torch.empty((int(L.fnp_sparse_to_dense_workspace_bytes(B, *shape)),), dtype=torch.uint8, device=cuda)
    f = torch.empty((idx.shape[0], C), dtype=torch.bfloat16, device=cuda)
    G = torch.empty((B, C, *shape), dtype=torch.bfloat16, device=cuda)
    new = lambda: (torch.randn(f.shape, device=cuda).to(f.dtype), torch.randn(G.shape, device=cuda).to(G.dtype))

    def run():
        return S.to_dense(f, idx, n_dev, B, list(shape), workspace=ws), S.dense_backward(G, idx, n_dev, B, shape, workspace=ws)

    a, b_ = new()
    f.copy_(a); G.copy_(b_)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    gc.collect()
    gc.disable()                          # (no collection inside the capture)
    try:
        with torch.cuda.graph(graph):
            dense_o, grad_o = run()
    finally:
        gc.enable()
    for _ in range(2):
        a, b_ = new()
        f.copy_(a); G.copy_(b_)
        graph.replay()
        want_d, want_g = run()
        torch.cuda.synchronize()
        assert torch.equal(dense_o, want_d) and torch.equal(grad_o, want_g)
        assert torch.equal(grad_o, S.dense_backward(G, idx, n_dev, B, shape))
