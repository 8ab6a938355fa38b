"""conv_out's own kernel (csrc/spconv_out128.hip: 128 -> 128 channels, kernel (3,1,1), stride (2,1,1), the three weight slabs resident in
LDS, independent waves) against the generic table kernel of csrc/spconv.hip.  Both run the same matrix instructions on the same operands
in the same order and the same epilogue arithmetic, so the outputs must be equal element for element: torch.equal, no tolerance.

fnp_spconv_forward takes the new kernel for K == 3, 128 -> 128, 16-bit input, no residual, from OUT128_MIN_CAP rows of capacity on.  The
generic kernel is reached through the same entry with a residual of zeros (outside the new dispatch; adding +0 changes no value), and
below the threshold by the plain call itself."""
import numpy as np
import pytest
import torch

from findnpropagate_amd import sparse as S

pytestmark = pytest.mark.gpu

C = 128
DEPTH = 5                          # z cells of the input grid: outputs z = 0 (inputs 0, 1, 2) and z = 1 (inputs 2, 3, 4)
OUT128_MIN_CAP = 256 * 8 * 64      # spconv.hip kOut128MinCap: 256 workgroups x 8 waves x two 32-row tiles
SENTINEL = 12288.0                 # (exact in bf16 and fp16)


def _sites(rng, B, H, W, fill=0.55, shuffle=False):
    """columns of 0 to 5 occupied z cells, rows [b, z, y, x]"""
    occ = rng.random((B, DEPTH, H, W)) < fill
    idx = np.argwhere(occ).astype(np.int32)
    if shuffle:
        idx = idx[rng.permutation(idx.shape[0])]
    return np.ascontiguousarray(idx)


# (name, scenes, H, W, rows in random order, capacity(m), rows the convolution is told of (m))
CASES = [
    # 40 x 40: ~5 k output rows in a capacity just above the threshold — most waves of the persistent grid own no rows
    ("small grid, spare capacity", 2, 40, 40, False, lambda m: OUT128_MIN_CAP + 37, lambda m: m),
    # ~61 k rows on either side of the dispatch threshold
    ("just below the threshold", 2, 130, 130, False, lambda m: OUT128_MIN_CAP - 1, lambda m: m),
    ("just above the threshold", 2, 130, 130, False, lambda m: OUT128_MIN_CAP, lambda m: m),
    # the range ends inside a 16-row block, and inside the first block of a wave's last tile
    ("rows end inside a block", 2, 130, 130, True, lambda m: OUT128_MIN_CAP + 4096, lambda m: (m // 32) * 32 - 32 + 5),
    # 200 x 200 x 4 scenes: ~290 k rows, several tiles per wave
    ("large, exact capacity", 4, 200, 200, False, lambda m: m, lambda m: m),
    ("large, spare capacity, odd rows", 3, 200, 200, True, lambda m: m + 5000, lambda m: m - 21),
]


@pytest.fixture(scope="module")
def weights(cuda):
    g = torch.Generator(device=cuda).manual_seed(99)
    w = torch.randn((C, 3, 1, 1, C), device=cuda, generator=g) * 0.05
    sc = torch.rand(C, device=cuda, generator=g) + 0.5
    sh = torch.randn(C, device=cuda, generator=g)
    return w, sc, sh


@pytest.mark.parametrize("name,B,H,W,shuffle,cap_of,n_of", CASES, ids=[c[0] for c in CASES])
def test_conv_out_equals_generic_kernel(cuda, rng, weights, name, B, H, W, shuffle, cap_of, n_of):
    idx = _sites(rng, B, H, W, shuffle=shuffle)
    n_in = idx.shape[0]
    d_idx = torch.from_numpy(idx).to(cuda)
    n_in_dev = S.device_scalar(n_in, cuda)
    grid = S.build_grid(d_idx, n_in_dev, B, [DEPTH, H, W])
    probe = S.rulebook_strided(d_idx, n_in_dev, grid, (3, 1, 1), (2, 1, 1), 0, cap_out=2 * B * H * W)
    m = int(probe.out_n.item())
    cap, n = cap_of(m), n_of(m)
    assert 0 < n <= m <= cap, (name, n, m, cap)
    rb = S.rulebook_strided(d_idx, n_in_dev, grid, (3, 1, 1), (2, 1, 1), 0, cap_out=cap)
    assert rb.K == 3 and rb.cap_out == cap and int(rb.out_n.item()) == m and rb.out_shape[0] == 2
    present = (rb.nbr[:, :m] >= 0).sum(0)
    assert set(present.unique().tolist()) == {1, 2, 3}, "outputs with one, two and three inputs"
    new_path = cap >= OUT128_MIN_CAP
    n_dev = S.device_scalar(n, cuda)
    w, sc, sh = weights
    g = torch.Generator(device=cuda).manual_seed(7)
    x32 = torch.randn((n_in, C), device=cuda, generator=g)
    for dtype in (torch.bfloat16, torch.float16):
        x, wp = x32.to(dtype), S.pack_weight(w, dtype)
        for out_dtype in (dtype, torch.float32):
            zeros = torch.zeros((cap, C), dtype=out_dtype, device=cuda)
            for scale, shift, relu in ((sc, sh, True), (None, None, False), (sc, sh, False), (None, None, True)):
                out = torch.full((cap, C), SENTINEL, dtype=out_dtype, device=cuda)
                S.conv_forward(x, wp, rb, n_dev, out_dtype=out_dtype, scale=scale, shift=shift, relu=relu, out=out)
                ref = S.conv_forward(x, wp, rb, n_dev, out_dtype=out_dtype, scale=scale, shift=shift, residual=zeros, relu=relu)
                what = (name, dtype, out_dtype, scale is not None, relu)
                assert torch.equal(out[:n], ref[:n]), what + (int((out[:n] != ref[:n]).any(1).sum().item()), "rows differ")
                if new_path:   # rows past the count stay untouched
                    assert bool((out[n:] == SENTINEL).all()), what
    # run to run: nothing in the kernel depends on timing
    a = S.conv_forward(x, wp, rb, n_dev, out_dtype=torch.float32, scale=sc, shift=sh, relu=True)
    b = S.conv_forward(x, wp, rb, n_dev, out_dtype=torch.float32, scale=sc, shift=sh, relu=True)
    assert torch.equal(a[:n], b[:n])
