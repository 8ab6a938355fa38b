"""BatchNorm2d (training mode) + ReLU on rows that stand for a dense BEV map, as ONE autograd node backed by csrc/bev_bn.hip
(fnp_bev_bn_train_forward / fnp_bev_bn_train_backward).

The rows are the output of a bias-free convolution on its output sites; every other cell of the (B, H, W) map holds an exact
zero.  The batch statistics of `nn.BatchNorm2d` run over ALL B * H * W cells, so the zeros enter mean and variance, end as
the per-channel constant relu(beta - mean * invstd * gamma) and, through it, take part in the gradients of gamma and beta.
`bev_bn_act` returns the dense (B, C, H, W) map the reference's `BatchNorm2d -> ReLU` would return on the dense convolution
output, in the rows' dtype; the normalised rows are never stored on their own.  It follows spconv.norm._BNActFunction."""
import torch
import torch.nn as nn

from .. import lib as _l

CHANNELS = (8, 16, 32, 64, 128, 256)


def channels_ok(C, dtype):
    """the kernels' shapes: a power of two in [8, 256] whose 64 staged rows fit 64 KB of LDS (256 channels: 16-bit rows only)"""
    return C in CHANNELS and not (C == 256 and dtype == torch.float32)


class _BevBNActFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, coords, n_dev, running_mean, running_var, batches_tracked, B, H, W, momentum, eps):
        L = _l.load()
        _l.require_device(x, coords, n_dev)
        assert x.is_contiguous() and x.dim() == 2 and coords.is_contiguous() and coords.dtype == torch.int32
        cap, C = x.shape
        assert cap >= 1 and coords.shape[0] >= cap and coords.shape[1] == 4
        dev = x.device
        y = torch.empty((B, C, H, W), dtype=x.dtype, device=dev)
        mean, invstd, fill = (torch.empty((C,), dtype=torch.float32, device=dev) for _ in range(3))
        # a workspace per call: a later forward must not rewrite what a pending backward needs (sparse.DenseFunction's note);
        # the backward rebuilds the cell -> row map in one of its own
        ws = torch.empty((int(L.fnp_bev_bn_workspace_bytes(C, B, H, W)),), dtype=torch.uint8, device=dev)
        g32, b32 = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        rc = L.fnp_bev_bn_train_forward(_l.ptr(x), _l.dtype_code(x), _l.ptr(coords), _l.ptr(n_dev), cap, C, B, H, W, _l.ptr(g32),
                                        _l.ptr(b32), _l.ptr(running_mean), _l.ptr(running_var), float(momentum), float(eps), _l.ptr(y),
                                        _l.ptr(mean), _l.ptr(invstd), _l.ptr(fill), _l.ptr(batches_tracked), _l.ptr(ws), ws.numel(),
                                        _l.stream())
        _l.check(rc, "fnp_bev_bn_train_forward")
        # the kernel wrote the buffers through raw pointers: tell torch (BaseBEVBackbone._prepare keys its eval fold on versions)
        if batches_tracked is not None:
            torch.autograd.graph.increment_version(batches_tracked)
        if running_mean is not None:
            torch.autograd.graph.increment_version(running_mean)
            torch.autograd.graph.increment_version(running_var)
        ctx.save_for_backward(x, coords, n_dev, g32, b32, mean, invstd, fill)
        ctx.geom, ctx.param_dtype = (B, H, W), gamma.dtype
        ctx.mark_non_differentiable(mean, invstd, fill)
        return y, mean, invstd, fill

    @staticmethod
    def backward(ctx, grad_out, _gm, _gi, _gf):
        L = _l.load()
        x, coords, n_dev, g32, b32, mean, invstd, fill = ctx.saved_tensors
        B, H, W = ctx.geom
        cap, C = x.shape
        grad_out = grad_out.contiguous().to(x.dtype)
        dx = torch.empty_like(x)
        dgamma = torch.empty((C,), dtype=torch.float32, device=x.device)
        dbeta = torch.empty((C,), dtype=torch.float32, device=x.device)
        ws = torch.empty((int(L.fnp_bev_bn_workspace_bytes(C, B, H, W)),), dtype=torch.uint8, device=x.device)
        rc = L.fnp_bev_bn_train_backward(_l.ptr(grad_out), _l.ptr(x), _l.dtype_code(x), _l.ptr(coords), _l.ptr(n_dev), cap, C, B, H, W,
                                         _l.ptr(g32), _l.ptr(b32), _l.ptr(mean), _l.ptr(invstd), _l.ptr(fill), _l.ptr(dx), _l.ptr(dgamma),
                                         _l.ptr(dbeta), _l.ptr(ws), ws.numel(), _l.stream())
        _l.check(rc, "fnp_bev_bn_train_backward")
        return (dx, dgamma.to(ctx.param_dtype), dbeta.to(ctx.param_dtype)) + (None,) * 10


def fusable(bn):
    """a plain affine nn.BatchNorm2d with a fixed momentum and running statistics (SyncBatchNorm is not one)"""
    return (type(bn) is nn.BatchNorm2d and bn.affine and bn.momentum is not None and bn.track_running_stats
            and bn.running_mean is not None)


def bev_bn_act(x, coords, n_dev, B, H, W, bn, stats=False):
    """relu(bn(map)) as a dense (B, C, H, W) tensor of x's dtype, where map holds the first n_dev rows of x (cap, C) on the sites
    coords (cap, 4) int32 [b, 0, y, x] and zeros elsewhere.  bn: nn.BatchNorm2d; its batch statistics run over the B * H * W
    cells, its running statistics and num_batches_tracked advance exactly like torch's training forward.  Differentiable in
    x, bn.weight and bn.bias.  stats=True: also (save_mean, save_invstd, fill), f32 (C,), not differentiable."""
    assert fusable(bn) and channels_ok(x.shape[1], x.dtype)
    nbt = bn.num_batches_tracked
    if not (nbt.is_cuda and nbt.dtype == torch.int64):
        with torch.no_grad():
            bn.num_batches_tracked += 1
        nbt = None
    y, mean, invstd, fill = _BevBNActFunction.apply(x.contiguous(), bn.weight, bn.bias, coords, n_dev, bn.running_mean, bn.running_var,
                                                    nbt, int(B), int(H), int(W), bn.momentum, bn.eps)
    return (y, mean, invstd, fill) if stats else y
