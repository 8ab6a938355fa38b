"""BaseBEVBackbone (pcdet/models/backbones_2d/base_bev_backbone.py:6-111) with its FIRST block evaluated on the sparse rows.

The reference densifies the encoded sparse tensor (HeightCompression: (B, 128, 2, 180, 180) -> (B, 256, 180, 180), 33 MB per
scene in f32 of which ~90 % are zeros) and runs `ZeroPad2d(1) -> Conv2d(256 -> 128, 3x3) -> BatchNorm2d -> ReLU` on it
(:31-40).  Here, in eval mode, that block reads the sparse rows directly:

  * the 2D convolution over (c, z) channels IS a 3D sparse convolution with a (2, 3, 3) kernel, stride 1, padding (0, 1, 1)
    whose output grid has one z plane: W3d[co, z, ky, kx, c] = W2d[co, c * D + z, ky, kx] (the view of height_compression.py:23
    puts channel c of plane z at c * D + z).  Its output sites are the BEV cells with at least one input row in their 3x3
    window; everything else sees only zeros and ends as relu(BatchNorm shift), a constant per channel;
  * so: rulebook of that convolution on the rank grid (fnp_rulebook_strided), the implicit-GEMM kernel with the BatchNorm
    (eval) scale / shift and the ReLU in its epilogue (fnp_spconv_forward: f32 rows on v_mfma_f32_16x16x4_f32, bf16 / fp16
    rows on v_mfma_f32_16x16x32), and ONE dense write of the (B, 128, 180, 180) result with relu(shift) in the cells without
    a row (fnp_sparse_to_dense_fill).  The 33 MB-per-scene map is never written or read, the matrix work covers the
    ~13 rows-in-reach per output cell instead of 9 x 256 dense taps.

The module tree (`blocks`, `deblocks`) — hence the state_dict keys — and forward(data_dict) are the reference's; training
mode, a first block that is not 3x3 / stride 1, or a data_dict without 'encoded_spconv_tensor' take the dense path through
the torch modules.  Remaining layers are the reference's dense torch modules (out of this path's scope).

Training (model cfg FNP_SPARSE_FIRST_TRAIN: True, opt-in; off: the dense torch path as ever).  The same block under autograd
without the dense input map: the rulebook as above, spconv.conv.SparseConvFunction (forward, data gradient, weight gradient)
on a differentiable (Cout, D, 3, 3, C) view of the Conv2d weight, so that autograd carries dW back into the Conv2d layout,
and bev_norm.bev_bn_act — BatchNorm2d with BATCH statistics over all B * H * W cells (the cells without a row are zeros of
the bias-free convolution and count), ReLU and the one dense write, forward and backward in csrc/bev_bn.hip.  Nothing on
this route reads a value back to the host.  sparse_train_reasons() says why a forward would take the dense path instead.
With HeightCompression's FNP_DEFER_DENSE the input map is not written at all: when this module needs it (dense path) and
finds no 'spatial_features', it densifies by itself."""
import numpy as np
import torch
import torch.nn as nn

from .. import sparse as S
from ..spconv.conv import SparseConvFunction
from . import bev_norm


def _get(cfg, key, default=None):
    if cfg is None:
        return default
    if hasattr(cfg, "get"):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


class BaseBEVBackbone(nn.Module):
    def __init__(self, model_cfg, input_channels):
        super().__init__()
        self.model_cfg = model_cfg
        layer_nums = list(_get(model_cfg, "LAYER_NUMS", None) or [])
        layer_strides = list(_get(model_cfg, "LAYER_STRIDES", None) or [])
        num_filters = list(_get(model_cfg, "NUM_FILTERS", None) or [])
        assert len(layer_nums) == len(layer_strides) == len(num_filters)
        upsample_strides = list(_get(model_cfg, "UPSAMPLE_STRIDES", None) or [])
        num_upsample_filters = list(_get(model_cfg, "NUM_UPSAMPLE_FILTERS", None) or [])
        assert len(upsample_strides) == len(num_upsample_filters)
        bn = lambda c: nn.BatchNorm2d(c, eps=1e-3, momentum=0.01)
        self.blocks, self.deblocks = nn.ModuleList(), nn.ModuleList()
        c_in = [input_channels] + num_filters[:-1]
        for i, (n_layers, stride, c_out) in enumerate(zip(layer_nums, layer_strides, num_filters)):
            layers = [nn.ZeroPad2d(1), nn.Conv2d(c_in[i], c_out, kernel_size=3, stride=stride, padding=0, bias=False), bn(c_out), nn.ReLU()]
            for _ in range(n_layers):
                layers += [nn.Conv2d(c_out, c_out, kernel_size=3, padding=1, bias=False), bn(c_out), nn.ReLU()]
            self.blocks.append(nn.Sequential(*layers))
            if upsample_strides:
                us = upsample_strides[i]
                if us > 1 or (us == 1 and not _get(model_cfg, "USE_CONV_FOR_NO_STRIDE", False)):
                    up = nn.ConvTranspose2d(c_out, num_upsample_filters[i], us, stride=us, bias=False)
                else:
                    ds = int(np.round(1 / us))
                    up = nn.Conv2d(c_out, num_upsample_filters[i], ds, stride=ds, bias=False)
                self.deblocks.append(nn.Sequential(up, bn(num_upsample_filters[i]), nn.ReLU()))
        c_cat = sum(num_upsample_filters)
        if len(upsample_strides) > len(layer_nums):
            self.deblocks.append(nn.Sequential(nn.ConvTranspose2d(c_cat, c_cat, upsample_strides[-1], stride=upsample_strides[-1], bias=False),
                                               bn(c_cat), nn.ReLU()))
        self.num_bev_features = c_cat
        # our additions (model cfg): FNP_SPARSE_FIRST (default True) — evaluate the first block on the sparse rows when it can;
        # FNP_BEV_DTYPE 'keep' (default: compute in the dtype of the encoded rows) | 'fp32' | 'bf16' | 'fp16'
        self.sparse_first = bool(_get(model_cfg, "FNP_SPARSE_FIRST", True))
        self.bev_dtype = {"keep": None, "fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[
            str(_get(model_cfg, "FNP_BEV_DTYPE", "keep")).lower()]
        # FNP_SPARSE_FIRST_TRAIN (default False): in train() the first block runs on the sparse rows under autograd
        self.sparse_first_train = bool(_get(model_cfg, "FNP_SPARSE_FIRST_TRAIN", False))
        self._prep = None
        self._ws = None
        self._dense_ws = None

    # ---------------------------------------------------------------- first block on sparse rows
    def _can_go_sparse(self, data_dict):
        if self.training or not self.sparse_first or len(self.blocks) == 0 or "encoded_spconv_tensor" not in data_dict:
            return False
        conv, t = self.blocks[0][1], data_dict["encoded_spconv_tensor"]
        return (tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (1, 1) and conv.bias is None and t.features.is_cuda
                and conv.in_channels == t.features.shape[1] * t.spatial_shape[0]
                and (t.features.shape[1], conv.out_channels) in S.F32_MFMA_SHAPES)

    def _prepare(self, D, dtype):
        """packed (K = D * 9, Cout, C) weight in `dtype` and the folded BatchNorm2d(eval) constants, cached on the parameters'
        versions.  The fold runs on the host in IEEE f32, as FusedResBackbone._fold does."""
        conv, bn = self.blocks[0][1], self.blocks[0][2]
        key = tuple((p.data_ptr(), p._version) for p in (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)) + (D, dtype)
        if self._prep is not None and self._prep[0] == key:
            return self._prep[1]
        c_out, c_in2d = conv.weight.shape[:2]
        w3 = conv.weight.detach().view(c_out, c_in2d // D, D, 3, 3).permute(0, 2, 3, 4, 1).contiguous()   # (Cout, kD, kH, kW, C)
        w = S.pack_weight(w3, dtype, mfma_f32=True)
        f32 = lambda t: t.detach().float().cpu().numpy()
        inv = np.float32(1.0) / np.sqrt(f32(bn.running_var) + np.float32(bn.eps))
        scale = f32(bn.weight) * inv
        shift = f32(bn.bias) - f32(bn.running_mean) * scale
        dev = conv.weight.device
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
        prep = (w, to(scale), to(shift), to(np.maximum(shift, np.float32(0.0))))
        self._prep = (key, prep)
        return prep

    def first_block_from_sparse(self, t):
        """encoded_spconv_tensor (rows (n, C) on a (D, H, W) grid) -> (B, Cout, H, W) f32: relu(bn(conv3x3(dense view)))."""
        D, H, W = t.spatial_shape
        B = t.batch_size
        feats = t.features.contiguous()
        dtype = self.bev_dtype or (feats.dtype if feats.dtype in (torch.float32, torch.bfloat16, torch.float16) else torch.float32)
        if feats.dtype != dtype:
            feats = feats.to(dtype)
        w, scale, shift, background = self._prepare(D, dtype)
        n_dev = t.n_dev()
        grid = t.rank_grid()
        cap_out = max(1, min(9 * max(feats.shape[0], 1), B * H * W))
        rb = S.rulebook_strided(t.indices, n_dev, grid, (D, 3, 3), 1, (0, 1, 1), cap_out)
        rows = S.conv_forward(feats, w, rb, rb.out_n, out_dtype=torch.float32, scale=scale, shift=shift, relu=True)
        need = int(S._l.load().fnp_sparse_to_dense_workspace_bytes(B, 1, H, W))
        if self._ws is None or self._ws.numel() < need or self._ws.device != feats.device:
            self._ws = torch.empty((need,), dtype=torch.uint8, device=feats.device)
        dense = S.to_dense(rows, rb.out_indices, rb.out_n, B, [1, H, W], workspace=self._ws, fill=background)
        return dense.view(B, rows.shape[1], H, W)

    # ---------------------------------------------------------------- first block on sparse rows, training
    def _rows_dtype(self, feats):
        """the computation dtype of the training route: FNP_BEV_DTYPE, else the autocast dtype (what autocast gives the dense
        route's Conv2d), else the rows' own"""
        if self.bev_dtype is not None:
            return self.bev_dtype
        if torch.is_autocast_enabled():
            return torch.get_autocast_gpu_dtype()
        return feats.dtype

    def sparse_train_reasons(self, data_dict):
        """why a training forward on `data_dict` would NOT take the first block from the sparse rows: a list of short strings,
        empty when the route can run.  (Says nothing about self.training: forward() asks only in train().)"""
        why = []
        if not self.sparse_first_train:
            why.append("FNP_SPARSE_FIRST_TRAIN is off")
        if len(self.blocks) == 0:
            return why + ["no blocks"]
        if "encoded_spconv_tensor" not in data_dict:
            return why + ["no encoded_spconv_tensor"]
        conv, bn, t = self.blocks[0][1], self.blocks[0][2], data_dict["encoded_spconv_tensor"]
        if not (tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (1, 1) and tuple(conv.dilation) == (1, 1) and conv.groups == 1):
            why.append("first block not 3x3 / stride 1")
        if conv.bias is not None:
            why.append("first convolution has a bias")
        if not bev_norm.fusable(bn):
            why.append("BatchNorm not a plain affine nn.BatchNorm2d with a fixed momentum and running statistics")
        feats = t.features
        if not (feats.is_cuda and conv.weight.is_cuda):
            why.append("not on the device")
        dtype = self._rows_dtype(feats)
        if dtype not in (torch.float32, torch.bfloat16, torch.float16):
            why.append("dtype %s not f32 / bf16 / fp16" % (dtype,))
        if feats.shape[0] == 0:
            why.append("no rows")
        C, D = feats.shape[1], int(t.spatial_shape[0])
        if conv.in_channels != C * D or (C, conv.out_channels) not in S.F32_MFMA_SHAPES or not bev_norm.channels_ok(conv.out_channels, dtype):
            why.append("(C, Cout) = (%d, %d) on %d planes outside the kernels' shapes" % (C, conv.out_channels, D))
        return why

    def first_block_train(self, t):
        """encoded_spconv_tensor -> (B, Cout, H, W) in the rows' dtype: relu(bn(conv3x3(dense view))) of the first block in
        training mode, under autograd (rows, conv.weight, bn.weight, bn.bias).  No host read: the output row count stays on
        the device, its capacity min(9 * rows, B * H * W) is known here."""
        conv, bn = self.blocks[0][1], self.blocks[0][2]
        D, H, W = (int(v) for v in t.spatial_shape)
        B = int(t.batch_size)
        feats = t.features
        dtype = self._rows_dtype(feats)
        if feats.dtype != dtype:
            feats = feats.to(dtype)
        feats = feats.contiguous()
        n_dev = t.n_dev()
        cap_out = max(1, min(9 * max(feats.shape[0], 1), B * H * W))
        rb = S.rulebook_strided(t.indices, n_dev, t.rank_grid(), (D, 3, 3), 1, (0, 1, 1), cap_out)
        c_out, c_in2d = conv.weight.shape[:2]
        w3 = conv.weight.view(c_out, c_in2d // D, D, 3, 3).permute(0, 2, 3, 4, 1)      # (Cout, kD, kH, kW, C): a view, differentiable
        rows = SparseConvFunction.apply(feats, w3, rb, rb.out_n, n_dev, False, None, None)
        return bev_norm.bev_bn_act(rows, rb.out_indices, rb.out_n, B, H, W, bn)

    def _dense_input(self, data_dict):
        """'spatial_features', or — HeightCompression with FNP_DEFER_DENSE left it out — the dense view of the encoded tensor,
        made here (differentiable when the rows require grad)"""
        if "spatial_features" in data_dict:
            return data_dict["spatial_features"]
        t = data_dict["encoded_spconv_tensor"]
        feats = t.features.contiguous()
        need = int(S._l.load().fnp_sparse_to_dense_workspace_bytes(t.batch_size, *t.spatial_shape))
        if self._dense_ws is None or self._dense_ws.numel() < need or self._dense_ws.device != feats.device:
            self._dense_ws = torch.empty((need,), dtype=torch.uint8, device=feats.device)
        dense = S.to_dense(feats, t.indices, t.n_dev(), t.batch_size, list(t.spatial_shape), workspace=self._dense_ws)
        N, C, D, H, W = dense.shape
        return dense.view(N, C * D, H, W)

    # ---------------------------------------------------------------- reference contract
    def forward(self, data_dict):
        """data_dict: 'spatial_features' (B, C*D, H, W) and / or 'encoded_spconv_tensor' -> 'spatial_features_2d'
        (+ 'spatial_features_%dx' per block), base_bev_backbone.py:82-111."""
        sparse = self._can_go_sparse(data_dict)
        sparse_train = self.training and self.sparse_first_train and not self.sparse_train_reasons(data_dict)
        if sparse or sparse_train:
            t = data_dict["encoded_spconv_tensor"]
            in_h = t.spatial_shape[1]
            x = None
        else:
            x = self._dense_input(data_dict)
            in_h = x.shape[2]
        ups, ret = [], {}
        for i, block in enumerate(self.blocks):
            if i == 0 and (sparse or sparse_train):
                x = self.first_block_train(t) if sparse_train else self.first_block_from_sparse(t)
                x = block[4:](x)
            else:
                x = block(x)
            ret["spatial_features_%dx" % int(in_h / x.shape[2])] = x
            ups.append(self.deblocks[i](x) if len(self.deblocks) > 0 else x)
        if len(ups) > 1:
            x = torch.cat(ups, dim=1)
        elif len(ups) == 1:
            x = ups[0]
        if len(self.deblocks) > len(self.blocks):
            x = self.deblocks[-1](x)
        # (the reference builds ret_dict and never stores it: only 'spatial_features_2d' is added)
        data_dict["spatial_features_2d"] = x
        return data_dict
