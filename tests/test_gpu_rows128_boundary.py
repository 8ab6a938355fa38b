"""The TILE BOUNDARIES of the class-sorted 128 -> 128 row pipeline (csrc/spconv_rows128.hip) against fnp_spconv_forward on the plain table:
torch.equal, no tolerance (same matrix instructions, operands, order and epilogue arithmetic).

What a tile's epilogue starts with — the rows behind the wave's positions (perm) and the NEXT tile's block masks and entry row — is
requested inside the tile's last kernel offset, whose two steps are peeled off the sweep loop.  The cases sit where that code can go
wrong: the next tile has another shape than this one (a full tile followed by a tail of one, two or three blocks per wave, or by
nothing), the last offset is also the first (isolated sites), consecutive tiles have different live offsets (a mixed batch), rows end
inside a block with spare capacity behind them; with and without residual, scale / shift and ReLU.  The residual holds a pattern that
names its row, so that a row fetched or stored through the wrong perm entry shows.

Geometry restated from csrc/sortedsweep.h and spconv.hip: from 32,768 rows of capacity the launch has 256 workgroups = 8 XCD groups of
32 slots; a group owns 1/8 of the 16-row blocks and sweeps them in rounds of 32 tiles of 384 rows (12,288 rows); what is left after the
full rounds is cut into 32 tiles of t blocks per wave, t = ceil(ceil(blocks left / 32) / 8), of which only the first few may exist."""
import numpy as np
import pytest
import torch

from findnpropagate_amd import sparse as S
from test_gpu_rows128 import C, ROWS128_MIN_CAP, TILE, _sites

pytestmark = pytest.mark.gpu

ROUND = 8 * 32 * TILE          # rows of one full round of all eight XCD groups: 98,304


def _tail_blocks(n):
    """blocks per wave of the partial round, per XCD group (csrc/sortedsweep.h fnp_xcd_rows / fnp_tail_blocks at 256 workgroups)"""
    nblk = (n + 15) // 16
    out = []
    for g in range(8):
        b0, b1 = (nblk * 32 * g) // 256, (nblk * 32 * (g + 1)) // 256
        rows = min(n, b1 * 16) - b0 * 16
        full = rows // (32 * TILE)
        per_slot = -(-((rows - full * 32 * TILE + 15) // 16) // 32)      # blocks of a slot's tail tile
        out.append((full, -(-per_slot // 8)))
    return out


# (kind, rows, spare capacity, expected (full rounds, tail blocks per wave) of every group or None)
CASES = [
    ("sheet", ROWS128_MIN_CAP + 2000, 0, None),            # just above the dispatch threshold: a partial round only, ragged end
    ("sheet", ROUND, 0, (1, 0)),                           # exactly one full tile per slot, nothing behind it
    ("sheet", ROUND + 8 * 1000, 0, (1, 1)),                # ... a one-block tail that only slots 0-7 of a group have
    ("sheet", ROUND + 8 * 6000, 0, (1, 2)),                # ... a two-block tail
    ("sheet", ROUND + 8 * 10000, 0, (1, 3)),               # ... a three-block tail (the full-tile form on a tail base)
    ("sheet", 150001, 30000, None),                        # rows end inside a block, spare capacity behind them
    ("lattice", 40000, 0, None),                           # isolated sites: the last offset is the first
    ("lattice", ROUND + 697, 0, None),                     # ... with a full round, a short tail and a ragged end
    ("mixed", 180000, 0, None),                            # consecutive tiles with different live offsets
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kind,n,spare,shape_want", CASES)
def test_rows128_tile_boundaries(cuda, rng, kind, n, spare, shape_want, dtype):
    if shape_want is not None:
        assert all(t == shape_want for t in _tail_blocks(n)), (n, _tail_blocks(n))
    idx, B, shape = _sites(rng, kind, n)
    if spare:
        idx = np.concatenate([idx, np.zeros((spare, 4), np.int32)])
    d_idx = torch.from_numpy(idx).to(cuda)
    n_dev = S.device_scalar(n, cuda)
    rb = S.rulebook_subm(d_idx, n_dev, S.build_grid(d_idx, n_dev, B, shape), 3)
    cap = rb.cap_out
    assert cap == n + spare and cap >= ROWS128_MIN_CAP
    g = torch.Generator(device=cuda).manual_seed(n)
    wp = S.pack_weight(torch.randn((C, 3, 3, 3, C), device=cuda, generator=g) * 0.05, dtype)
    x = torch.randn((cap, C), device=cuda, generator=g).to(dtype)
    sc = torch.rand(C, device=cuda, generator=g) + 0.5
    sh = torch.randn(C, device=cuda, generator=g)
    # residual row r: ((37 r) mod 255 - 127) / 4 in every channel, + c / 64 (then rounded to the 16-bit type; both kernels read the same tensor)
    r = torch.arange(cap, device=cuda)
    res = ((((r * 37) % 255) - 127).float() / 4)[:, None] + torch.arange(C, device=cuda).float()[None, :] / 64
    res = res.to(dtype)
    forms = ((None, sc, sh, True), (res, sc, sh, True), (res, None, None, False), (None, None, None, False), (res, sc, sh, False),
             (None, sc, sh, False), (res, None, None, True))
    plain = [S.conv_forward(x, wp, rb, n_dev, scale=a, shift=b, residual=rr, relu=relu, ranked=True) for rr, a, b, relu in forms]
    S.classsort(rb, n_dev, C)
    srt = [S.conv_forward(x, wp, rb, n_dev, scale=a, shift=b, residual=rr, relu=relu, ranked=True) for rr, a, b, relu in forms]
    for i, (a, b) in enumerate(zip(plain, srt)):
        assert torch.equal(a[:n], b[:n]), (kind, n, dtype, "form", i, int((a[:n] != b[:n]).any(1).sum().item()), "rows differ")
