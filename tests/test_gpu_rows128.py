"""The LDS-DMA row pipeline of the class-sorted 128 -> 128 sweep (csrc/spconv_rows128.hip) against fnp_spconv_forward on the plain
table.  Both run the same matrix instructions on the same operands in the same order, so the outputs must be the same bits:
torch.equal, no tolerance.  fnp_spconv_forward_sorted takes the new kernel from ROWS128_MIN_CAP rows of capacity on and the
register-pipeline kernel below; the cases sit on both sides."""
import numpy as np
import pytest
import torch

from findnpropagate_amd import sparse as S

pytestmark = pytest.mark.gpu

C = 128
TILE = 8 * 3 * 16              # rows of a workgroup tile: 8 waves x 3 blocks x 16
ROWS128_MIN_CAP = 256 * 8 * 16   # capacity from which the sorted sweep takes the row pipeline (spconv.hip, fnp_spconv_forward_sorted)


def _sheet(rng, B, shape, keep=0.8):
    """a two-cell-thick wavy sheet per scene (see tests/test_gpu_spconv.py): most sites have neighbours in one adjacent z plane only"""
    D, H, W = shape
    out = []
    for b in range(B):
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        z0 = ((D - 2) * 0.5 * (1 + np.sin(yy / 7.0 + b) * np.cos(xx / 9.0))).astype(np.int64).clip(0, D - 2)
        for dz in (0, 1):
            k = rng.random((H, W)) < keep
            out.append(np.stack([np.full(k.sum(), b), (z0 + dz)[k], yy[k], xx[k]], 1))
    return np.concatenate(out).astype(np.int32)


def _lattice(b, shape):
    """every second cell in z, y and x of scene b: no site has a neighbour but itself (only the centre offset is live)"""
    D, H, W = shape
    zz, yy, xx = np.meshgrid(np.arange(0, D, 2), np.arange(0, H, 2), np.arange(0, W, 2), indexing="ij")
    return np.stack([np.full(zz.size, b), zz.ravel(), yy.ravel(), xx.ravel()], 1).astype(np.int32)


def _sites(rng, kind, n):
    if kind == "sheet":         # B = 4 scenes of 5 x 200 x 200: up to ~256 k sites
        B, shape = 4, [5, 200, 200]
        idx = _sheet(rng, B, shape)
        idx = idx[rng.permutation(idx.shape[0])[:n]]
        idx = idx[np.lexsort((idx[:, 1], idx[:, 3], idx[:, 2], idx[:, 0]))]
    elif kind == "lattice":     # isolated sites only: every tile has every offset dead but the centre
        B, shape = 2, [9, 200, 200]
        idx = np.concatenate([_lattice(b, shape) for b in range(B)])
        idx = idx[rng.permutation(idx.shape[0])[:n]]
    else:                       # "mixed": scenes 0-1 a sheet, scenes 2-3 isolated sites, rows in random order
        B, shape = 4, [9, 200, 200]
        a = _sheet(rng, 2, shape)
        idx = np.concatenate([a, _lattice(2, shape), _lattice(3, shape)])
        idx = idx[rng.permutation(idx.shape[0])[:n]]
    assert idx.shape[0] == n, (kind, n, idx.shape[0])
    return idx, B, shape


# (kind, rows, spare capacity behind the rows)
CASES = [
    ("sheet", ROWS128_MIN_CAP - 2768, 0),       # below the dispatch threshold: the register pipeline
    ("sheet", ROWS128_MIN_CAP + 16, 0),         # just above: one block per wave, a partial round only
    ("sheet", 60001, 0),                        # partial round of two-block tiles, n not a multiple of 16
    ("sheet", 256 * TILE + 37, 0),              # one full round, then a partial round most slots have no tile of
    ("sheet", 2 * 256 * TILE + 24 * TILE + 5, 0),   # two full rounds + a partial one
    ("sheet", 150000, 50000),                   # capacity well above the rows (the grid is cut from the capacity, the rows from n)
    ("lattice", 70000, 0),                      # every (tile, offset) pair dead but the centre; all neighbours absent
    ("mixed", 180000, 0),                       # isolated rows among connected ones
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kind,n,spare", CASES)
def test_rows128_equals_plain_sweep(cuda, rng, kind, n, spare, dtype):
    idx, B, shape = _sites(rng, kind, n)
    if spare:
        idx = np.concatenate([idx, np.zeros((spare, 4), np.int32)])
    d_idx = torch.from_numpy(idx).to(cuda)
    n_dev = S.device_scalar(n, cuda)
    rb = S.rulebook_subm(d_idx, n_dev, S.build_grid(d_idx, n_dev, B, shape), 3)
    assert rb.cap_out == n + spare
    cap = rb.cap_out
    wp = S.pack_weight(torch.from_numpy((rng.standard_normal((C, 3, 3, 3, C)) * 0.05).astype(np.float32)).to(cuda), dtype)
    x = torch.from_numpy(rng.standard_normal((cap, C)).astype(np.float32)).to(cuda).to(dtype)
    sc = torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32)).to(cuda)
    sh = torch.from_numpy(rng.standard_normal(C).astype(np.float32)).to(cuda)
    res = torch.from_numpy(rng.standard_normal((cap, C)).astype(np.float32)).to(cuda).to(dtype)
    forms = ((None, sc, sh, True), (res, sc, sh, True), (res, None, None, False), (None, None, None, False), (None, sc, sh, False))
    plain = [S.conv_forward(x, wp, rb, n_dev, scale=a, shift=b, residual=r, relu=relu, ranked=True) for r, a, b, relu in forms]
    S.classsort(rb, n_dev, C)
    nbr = rb.nbr[:, :n].cpu().numpy()
    if kind == "lattice":
        assert (nbr[13] == np.arange(n)).all() and (np.delete(nbr, 13, 0) < 0).all(), "isolated sites: the centre only"
        assert (rb._sorted[1][:(n + 15) // 16].cpu().numpy().view(np.uint32) == 1 << 13).all()
    if kind == "mixed":
        lonely = (np.delete(nbr, 13, 0) < 0).all(0)
        assert 0.2 < lonely.mean() < 0.8
    srt = [S.conv_forward(x, wp, rb, n_dev, scale=a, shift=b, residual=r, relu=relu, ranked=True) for r, a, b, relu in forms]
    for i, (a, b) in enumerate(zip(plain, srt)):
        assert torch.equal(a[:n], b[:n]), (kind, n, dtype, "form", i, int((a[:n] != b[:n]).any(1).sum().item()), "rows differ")
    # run to run: the pipeline's waits are counted, not timed — a second sweep of the same inputs gives the same bits
    again = S.conv_forward(x, wp, rb, n_dev, scale=sc, shift=sh, residual=res, relu=True, ranked=True)
    assert torch.equal(again[:n], srt[1][:n])
