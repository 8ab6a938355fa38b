"""tests/ref_bev.py on the CPU: its two routes to the first BEV block agree, the checks the GPU tests apply reject planted
defects (and pass what is right), and the site sets of tests/test_gpu_bev_at_scale.py reach the forms they are written for —
known here, before a GPU is involved."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ref32 as R32
import ref64 as R
import ref_bev as RB

F32, BF16, FP16 = torch.float32, torch.bfloat16, torch.float16
ROUND_ROWS_128 = 256 * 8 * 3 * 16     # one round of the 128 -> 128 persistent grid of the 16-bit kernel (test_gpu_conv_at_scale.round_rows)


def _bn(rng, c=128):
    """BatchNorm2d statistics as tests/test_gpu_bev.py's `_net` draws them"""
    f = lambda a: a.astype(np.float32)
    return SimpleNamespace(weight=f(rng.uniform(0.5, 1.5, c)), bias=f(rng.standard_normal(c) * 0.3), running_mean=f(rng.standard_normal(c) * 0.2),
                           running_var=f(rng.uniform(0.5, 1.5, c)), eps=1e-3)


def _small(D, H, W, B=2, seed=0):
    rng = np.random.default_rng(seed)
    idx = RB.clustered(rng, B, (D, H, W), 400)
    x = rng.standard_normal((idx.shape[0], 128)).astype(np.float32)
    w2d = RB.stable_weight((rng.standard_normal((128, 128 * D, 3, 3)) * 0.05).astype(np.float32))
    return idx, x, w2d, _bn(rng), B, (D, H, W)


SMALL = {"D=2 37x41": (2, 37, 41), "D=1 24x24": (1, 24, 24)}


@pytest.mark.parametrize("name", list(SMALL))
def test_rows_reference_scattered_equals_the_dense_route(name):
    """f32 inputs, the float64 fold on both sides: the coordinate-derived rows placed on their sites and max(shift, 0) elsewhere
    equal torch's float64 conv2d + BatchNorm2d + ReLU on the (B, C * D, H, W) map to float64 rounding"""
    idx, x, w2d, bn, B, shape = _small(*SMALL[name])
    D, H, W = shape
    f = RB.folded(bn)
    out, V, e = RB.rows_reference(idx, x, B, shape, RB.weight3d(w2d, D), f.scale64, f.shift64, F32)
    assert 0 < out.shape[0] < B * H * W and (out[:, 1] == 0).all()
    a = torch.from_numpy(RB.scatter(out, V.numpy(), f.background64, B, H, W))
    b = RB.dense_reference(idx, x, B, shape, w2d, bn)
    assert a.shape == b.shape == (B, 128, H, W)
    # ~ 13 * 128 terms of magnitude <= |x| |w| |scale|: 2^-52 per operation, a few thousand operations
    tol = 1e-12 * max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= tol, float((a - b).abs().max())
    assert float(b.abs().max()) > 0.5 and bool((b[:, f.shift64 < 0] == 0).any())


def _planted(td, D, H, W):
    """a small case in `td`: reference, the f32 evaluation of the right table, and what a defect is applied to"""
    idx, x, w2d, bn, B, shape = _small(D, H, W, seed=3)
    f = RB.folded(bn)
    wp = RB.weight3d(w2d, D)
    if td != F32:
        x, wp = R.round16(x, td), R.round16(wp, td)
    out, nbr = RB.neighbours(idx, B, shape)
    _, V, e = RB.rows_reference(idx, x, B, shape, wp, f.scale, f.shift, td, tab=(out, nbr))
    ev = RB.evaluate_once_rounded if td == F32 else RB.evaluate32
    return SimpleNamespace(idx=idx, x=x, wp=wp, f=f, out=out, nbr=nbr, V=V, e=e, B=B, H=H, W=W, D=D, ev=ev,
                           dense=lambda rows: RB.scatter(out, rows, f.background, B, H, W))


def _rejected(c, dense):
    return RB.check_dense(dense, c.out, c.V, c.e, c.f.background)[1]


TYPES = [F32, BF16, FP16]
IDS = ["f32", "bf16", "fp16"]


@pytest.mark.parametrize("td", TYPES, ids=IDS)
def test_checks_pass_the_unplanted_evaluation(td):
    for D, H, W in SMALL.values():
        c = _planted(td, D, H, W)
        rows = c.ev(c.x, c.wp, c.nbr, c.f.scale, c.f.shift)
        assert rows.dtype == np.float32
        worst, fail = RB.check_dense(c.dense(rows), c.out, c.V, c.e, c.f.background)
        assert not fail and worst < 1.0, (worst, fail)


@pytest.mark.parametrize("td", TYPES, ids=IDS)
@pytest.mark.parametrize("k", [0, 8, 9, 17])
def test_checks_reject_one_dropped_neighbour(td, k):
    """one entry of the table of ONE row lost, at the first and last offset of each z plane; the row with the most neighbours
    that has one at k (the lost term is then the smallest share of its sum)"""
    c = _planted(td, 2, 37, 41)
    cand = np.nonzero(c.nbr[k] >= 0)[0]
    o = cand[np.argmax((c.nbr[:, cand] >= 0).sum(0))]
    assert (c.nbr[:, o] >= 0).sum() >= 4
    nbr = c.nbr.copy()
    nbr[k, o] = -1
    fail = _rejected(c, c.dense(c.ev(c.x, c.wp, nbr, c.f.scale, c.f.shift)))
    assert len(fail) == 1 and fail[0].startswith("rows: 1 of "), fail


@pytest.mark.parametrize("td", TYPES, ids=IDS)
def test_checks_reject_swapped_z_planes_of_the_weight(td):
    c = _planted(td, 2, 37, 41)
    swapped = np.ascontiguousarray(c.wp.reshape(2, 9, 128, 128)[::-1]).reshape(18, 128, 128)
    assert _rejected(c, c.dense(c.ev(c.x, swapped, c.nbr, c.f.scale, c.f.shift)))


@pytest.mark.parametrize("td", TYPES, ids=IDS)
def test_checks_reject_the_skipped_last_offset_of_odd_k(td):
    """K = 9 walked in pairs with the odd tail forgotten: offset 8 contributes nothing"""
    c = _planted(td, 1, 24, 24)
    assert c.nbr.shape[0] == 9 and (c.nbr[8] >= 0).any()
    nbr = c.nbr.copy()
    nbr[8] = -1
    assert _rejected(c, c.dense(c.ev(c.x, c.wp, nbr, c.f.scale, c.f.shift)))


def _background_cell(c):
    site = np.zeros((c.B, c.H, c.W), bool)
    site[c.out[:, 0], c.out[:, 2], c.out[:, 3]] = True
    cells = np.argwhere(~site)
    assert cells.shape[0]
    return site, cells


def test_checks_reject_shift_in_place_of_relu_shift_in_one_cell():
    c = _planted(F32, 2, 37, 41)
    good = c.dense(c.ev(c.x, c.wp, c.nbr, c.f.scale, c.f.shift))
    _, cells = _background_cell(c)
    b, y, x = cells[len(cells) // 2]
    ch = int(np.nonzero(c.f.shift < 0)[0][0])
    bad = good.copy()
    bad[b, ch, y, x] = c.f.shift[ch]
    fail = _rejected(c, bad)
    assert len(fail) == 1 and fail[0].startswith("background: 1 of "), fail
    # ... and a background that is right to 1e-6 but not in its bits (what allclose(atol=1e-6) lets through)
    ch = int(np.nonzero(c.f.shift > 0)[0][0])
    bad = good.copy()
    bad[b, ch, y, x] = np.nextafter(good[b, ch, y, x], np.float32(2.0))
    assert _rejected(c, bad)
    assert not _rejected(c, good)


def test_checks_reject_zero_in_place_of_the_background():
    c = _planted(F32, 2, 37, 41)
    good = c.dense(c.ev(c.x, c.wp, c.nbr, c.f.scale, c.f.shift))
    _, cells = _background_cell(c)
    b, y, x = cells[0]
    bad = good.copy()
    bad[b, :, y, x] = 0.0
    assert (c.f.background > 0).any() and _rejected(c, bad)


def test_checks_reject_a_row_written_to_the_neighbouring_cell():
    c = _planted(F32, 2, 37, 41)
    good = c.dense(c.ev(c.x, c.wp, c.nbr, c.f.scale, c.f.shift))
    site, _ = _background_cell(c)
    # an output site whose right neighbour is a cell without a row, and one whose right neighbour is another site
    for want_site in (False, True):
        pick = [o for o in c.out if o[3] + 1 < c.W and site[o[0], o[2], o[3] + 1] == want_site][0]
        b, _, y, x = pick
        bad = good.copy()
        bad[b, :, y, x + 1] = good[b, :, y, x]
        bad[b, :, y, x] = c.f.background if not want_site else good[b, :, y, x + 1]
        fail = _rejected(c, bad)
        assert fail and fail[0].startswith("rows: "), fail
        assert want_site or len(fail) == 2


def test_fold_restatement_is_within_its_bound_of_the_float64_fold():
    """4 * 2^-24 relative (the shift measured against |bias| + |mean * scale|), on the statistics the GPU tests draw"""
    f = RB.folded(_bn(np.random.default_rng(1234)))
    u4 = 4 * 2.0 ** -24
    assert (np.abs(f.scale - f.scale64) <= u4 * np.abs(f.scale64)).all()
    assert (np.abs(f.shift - f.shift64) <= u4 * f.bias_mag).all()
    assert (f.shift < 0).any() and (f.shift > 0).any()
    assert np.array_equal(f.background, np.where(f.shift > 0, f.shift, np.float32(0.0)))


def test_weight3d_is_the_docstrings_mapping():
    rng = np.random.default_rng(0)
    for D in (1, 2):
        w2d = rng.standard_normal((8, 16 * D, 3, 3)).astype(np.float32)
        wp = RB.weight3d(w2d, D)
        assert wp.shape == (D * 9, 8, 16)
        for co, c, z, ky, kx in [(0, 0, 0, 0, 0), (7, 15, D - 1, 2, 2), (3, 5, D - 1, 1, 0), (2, 9, 0, 0, 2)]:
            assert wp[(z * 3 + ky) * 3 + kx, co, c] == w2d[co, c * D + z, ky, kx]
    w = rng.standard_normal((18, 4, 32)).astype(np.float32)
    perm = w.reshape(18, 4, 2, 4, 4).transpose(0, 1, 2, 4, 3).reshape(18, 4, 32)      # position 4q + r <- channel 4r + q
    assert perm[0, 0, 4 * 1 + 2] == w[0, 0, 4 * 2 + 1] and np.array_equal(RB.unpermute(perm), w)
    s = RB.stable_weight(np.array([2.0 ** -14, -2.0 ** -13, 1e-3, -6e-5], np.float32))
    assert s.tolist() == [0.0, -2.0 ** -13, np.float32(1e-3), 0.0]
    for td in (BF16, FP16):      # what is left casts to the type exactly as round16 rounds it
        big = RB.stable_weight((rng.standard_normal(100000) * 1e-3).astype(np.float32))
        assert np.array_equal(R.round16(big, td), torch.from_numpy(big).to(td).float().numpy())


# ------------------------------------------------------------------------------------------------ the site sets
def _case(name):
    idx, B, (D, H, W) = RB.sites(name)
    out, nbr = RB.table(name)
    n = idx.shape[0]
    assert nbr.shape == (D * 9, out.shape[0]) and (nbr >= 0).any(0).all() and nbr.max() == n - 1
    assert out.shape[0] <= RB.cap_out_of(n, B, H, W)
    return idx, n, out, nbr, B, D, H, W, RB.cap_out_of(n, B, H, W), RB.tile_classes(out, B, H, W)


def test_site_set_corner():
    idx, n, out, nbr, B, D, H, W, cap, tc = _case("corner")
    assert (B, D, H, W) == (1, 2, 24, 24) and idx.tolist() == [[0, 1, 0, 0], [0, 0, 23, 23]]
    assert sorted(map(tuple, out[:, 2:].tolist())) == [(0, 0), (0, 1), (1, 0), (1, 1), (22, 22), (22, 23), (23, 22), (23, 23)]      # windows cut at the border
    assert (nbr >= 0).sum() == 8 and set(np.nonzero(nbr >= 0)[0]) == {9 + 4, 9 + 3, 9 + 1, 9 + 0, 8, 7, 5, 4}


def test_site_set_d1_odd():
    idx, n, out, nbr, B, D, H, W, cap, tc = _case("d1-odd")
    assert (B, D, H, W) == (2, 1, 37, 41) and nbr.shape[0] == 9 and (H * W) % 2 == 1 and tc["tile"] == 64 and tc["partial"]
    have = set(map(tuple, idx.tolist()))
    assert {(0, 0, 0, 0), (0, 0, 36, 40), (1, 0, 0, 40), (1, 0, 36, 0)} <= have
    assert tc["slots"] > 0 and not np.array_equal(idx, idx[np.lexsort(idx.T[::-1])])       # rows in random order
    assert (nbr[8] >= 0).any() and out.shape[0] % 16


def test_site_set_isolated():
    idx, n, out, nbr, B, D, H, W, cap, tc = _case("isolated")
    assert (B, D, H, W) == (2, 2, 40, 40) and out.shape[0] == 9 * n == cap < B * H * W
    assert ((nbr >= 0).sum(0) == 1).all() and set(idx[:, 1].tolist()) == {0, 1}


def test_site_set_solid():
    idx, n, out, nbr, B, D, H, W, cap, tc = _case("solid")
    assert (B, D, H, W) == (1, 2, 48, 48) and out.shape[0] == cap == B * H * W and n == H * W + H * W // 3
    assert tc["empty"] == tc["slots"] == 0 and tc["over"] == H * W // 128 and not tc["partial"]
    assert int((nbr >= 0).sum(0).max()) > 9      # both z planes feed one output


def test_site_set_mid():
    idx, n, out, nbr, B, D, H, W, cap, tc = _case("mid")
    assert (B, D, H, W) == (2, 2, 180, 180) and 8000 <= n <= 10000
    assert cap < ROUND_ROWS_128 and cap < R32.full_tile_cap(128)       # the evenly cut short ranges, under either kernel
    assert R32.grid_of(cap, 128) == R32.resident(128) and -(-cap // R32.tile_rows(128)) < R32.resident(128)      # (f32: ranges shorter than a tile)
    assert tc["empty"] > 0 and tc["slots"] > 0 and tc["over"] > 0 and tc["partial"] and tc["tile"] == 128 and H * W == 253 * 128 + 16


def test_site_set_full():
    idx, n, out, nbr, B, D, H, W, cap, tc = _case("full")
    m = out.shape[0]
    assert (B, D, H, W) == (8, 2, 180, 180)
    assert m >= 2 * ROUND_ROWS_128 + 16 * 1024 and m % 16 != 0            # two rounds and a partial one
    assert cap > 256 * 8 * 3 * 16 and cap > R32.full_tile_cap(128) and cap == B * H * W
    assert tc["over"] > 10 * (tc["slots"] + tc["empty"])                   # behind a 3 x 3 dilation most tiles exceed the LDS slots
    assert not np.array_equal(idx, idx[np.lexsort(idx.T[::-1])])
    # B = 7 at this occupancy stays under two rounds: 8 is the smallest batch of the case
    assert 7 * H * W * (1 - (1 - RB.FULL_OCCUPANCY) ** 9) < 2 * ROUND_ROWS_128
