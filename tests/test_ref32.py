"""tests/ref32.py, what the at-scale tests of the f32 engine (tests/test_gpu_f32_at_scale.py) add to tests/ref64.py, checked on the
CPU: the C oracle's f32 results lie inside the derived f32 bound and equal the float64 reference bit for bit on integer inputs,
forward and backward, for every channel pair and geometry of the backbone; the subset helper returns the bits of the full oracle
call; the restated launch geometry gives the constants the kernels' launch code gives; and PLANTED DEFECTS — what a subtly wrong
f32 kernel would write, applied to a correct f32 result — are each rejected by the comparators the GPU file uses: by the bound on
random data and by the bit-for-bit comparison on integer data."""
import numpy as np
import pytest
import torch

import ref32 as R32
import ref64 as R
from test_gpu_rows128 import _sheet

PAIRS = [(5, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128)]
GEOMS = [(3, 2, 1), (3, 2, (0, 1, 1)), ((3, 1, 1), (2, 1, 1), 0)]      # (k, s, p) of the backbone's strided layers
FORMS = [(False, False, False), (False, True, True), (True, True, True), (True, False, False)]   # (residual, scale / shift, relu)
ZERO = lambda V: torch.zeros_like(torch.as_tensor(V))


def _random_sites(rng, B, shape, n):
    cells = B * shape[0] * shape[1] * shape[2]
    lin = rng.choice(cells, size=n, replace=False)
    b, rem = np.divmod(lin, shape[0] * shape[1] * shape[2])
    z, rem = np.divmod(rem, shape[1] * shape[2])
    y, x = np.divmod(rem, shape[2])
    return np.stack([b, z, y, x], 1).astype(np.int32)


def _form(sums, d, form, out_dtype=torch.float32):
    res, scaled, relu = form
    return R32.epilogue(sums, d["sc"] if scaled else None, d["sh"] if scaled else None, d["res"] if res else None, relu, out_dtype)


def _oracle_form(oracle, y, d, form):
    res, scaled, relu = form
    if not (res or scaled or relu):
        return y
    return oracle.scale_shift_act(y, d["sc"] if scaled else None, d["sh"] if scaled else None, d["res"] if res else None, relu=relu)


# ------------------------------------------------------------------------------------------------ geometry
def test_restated_geometry_gives_the_constants_of_the_launch_code():
    assert [R32.tile_rows(c) for c in (16, 32, 64, 128)] == [256, 256, 256, 192]
    assert [R32.resident(c) for c in (16, 32, 64, 128)] == [1024, 1024, 512, 512]
    assert [R32.full_tile_cap(c) for c in (16, 32, 64, 128)] == [262144, 262144, 131072, 98304]
    # the grid: the persistent one from a capacity of `resident` 64-row quarters on, finer below
    assert R32.grid_of(1500, 16) == 24 and R32.grid_of(60000, 16) == 938 and R32.grid_of(65536, 16) == 1024 and R32.grid_of(32768, 64) == 512
    for cout in (16, 64, 128):
        assert R32.grid_of(R32.full_tile_cap(cout), cout) == R32.resident(cout) == R32.grid_of(10 ** 7, cout)
    # the class sort places q = 2 rows per thread from 1024 * grid rows on
    assert int(R32.sort_q(1048576, 1024).max()) == 1 and int(R32.sort_q(1048576 + 16, 1024).max()) == 2
    assert int(R32.sort_q(524288, 512).max()) == 1 and int(R32.sort_q(524288 + 16, 512).max()) == 2
    assert R32.FIRST_ROUND_ROWS == 524288
    # the range split: every row in exactly one range, whole blocks, every workgroup another range
    for n, G in [(1, 1024), (17, 512), (400, 512), (81909, 1024), (603397, 1024), (226000 + 5, 512), (949, 12), (5000, 13)]:
        rb, re = R32.ranges(n, G)
        assert rb[0] == 0 and re[-1] == n and (rb[1:] == np.maximum(re[:-1], rb[1:])).all() and (rb % 16 == 0).all()
        assert (re[:-1] % 16 == 0).all() and (re >= rb).all()
        assert sorted(R32.range_of_block(b, G) for b in range(G)) == list(range(G))
    assert R32.xcd_first(1024) == [128 * x for x in range(8)] and R32.xcd_first(13) == [0, 2, 4, 6, 8, 10, 11, 12]
    # a workgroup's waves: a short range is cut evenly (bpw blocks per wave, the last waves short or empty), a long one in tiles
    small, bpw, plan = R32.wave_plan(160, 160 + 5 * 16 - 11, 64)
    assert small and bpw == 2 and plan == [[(160, 192)], [(192, 224)], [(224, 229)], []]
    small, bpw, plan = R32.wave_plan(0, 11 * 16, 128)
    assert small and bpw == 3 and plan == [[(0, 48)], [(48, 96)], [(96, 144)], [(144, 176)]]
    small, bpw, plan = R32.wave_plan(0, 15 * 16, 16)
    assert small and bpw == 4 and [p[0][1] - p[0][0] for p in plan] == [64, 64, 64, 48]
    small, _, plan = R32.wave_plan(256, 256 + 600, 64)
    assert not small and plan == [[(256, 320), (512, 576), (768, 832)], [(320, 384), (576, 640), (832, 856)], [(384, 448), (640, 704)],
                                  [(448, 512), (704, 768)]]
    small, _, plan = R32.wave_plan(0, 192, 128)
    assert not small and plan == [[(0, 48)], [(48, 96)], [(96, 144)], [(144, 192)]]
    # weight gradient: chunks from the capacity, their borders from n
    assert [R32.wgrad_max_chunks(*p) for p in ((5, 16), (16, 16), (64, 64), (64, 128), (128, 128))] == [128, 32, 32, 32, 24]
    assert [R32.wgrad_pmax(*p) for p in ((5, 16), (16, 16), (64, 64), (64, 128), (128, 128))] == [0, 4, 16, 64, 64]
    assert R32.wgrad_chunks(1500, 16, 16) == 1 and R32.wgrad_chunks(5000, 64, 64) == 3 and R32.wgrad_chunks(65536, 64, 64) == 32
    assert R32.wgrad_chunks(49152, 128, 128) == 24 and R32.wgrad_chunks(262144, 5, 16) == 128 and R32.wgrad_chunks(10 ** 6, 16, 16) == 32
    assert R32.wgrad_rows_per_chunk(66536, 32) == 2176 and R32.wgrad_rows_per_chunk(36901, 32) == 1280 and R32.wgrad_live_chunks(36901, 32) == 29
    assert R32.wgrad_partials(66536, 64, 64, 27, False) == 32 and R32.wgrad_partials(263000, 5, 16, 27, False) == 128 * 4 + 11
    assert R32.wgrad_partials(263000, 5, 16, 27, True) == 128 * 27 * 4 + 11


def test_gamma_is_the_textbook_constant():
    assert R32.gamma(0) == 0.0 and abs(R32.gamma(3456) / (3456 * 2.0 ** -24) - 1) < 3e-4
    assert R32.gamma(100, 28) == R32.gamma(128) and R32.gamma(128) > 128 * 2.0 ** -24


def test_chain_rows_cover_what_they_promise(rng):
    cout, G = 64, 512
    n = 2 * R32.full_tile_cap(cout) + 39317
    rows = R32.chain_rows(n, cout, G, rng)
    assert 1500 < rows.shape[0] < 6000 and (np.diff(rows) > 0).all()
    rb, re = R32.ranges(n, G)
    have = set(rows.tolist())
    assert set(range(n // 16 * 16, n)) <= have and set(range(16)) <= have
    for f in R32.xcd_first(G)[1:]:
        assert {int(re[f - 1]) - 1, int(rb[f]), int(rb[f]) + 15} <= have
    b = int(rb[-1])
    assert {b + 255, b + 256, b + 64, b + 63, b + 512, b + 511} <= have
    thin = R32.chain_rows(17, cout, G, rng)
    assert thin.tolist() == list(range(17))


# ------------------------------------------------------------------------------------------------ the oracle inside the bound
@pytest.mark.parametrize("Cin,Cout", PAIRS)
def test_oracle_subm_inside_the_f32_bound_and_exact_on_integers(oracle, rng, Cin, Cout):
    B, shape, n = 2, [7, 16, 17], 1200
    idx = _random_sites(rng, B, shape, n)
    nbr = R.neighbours_subm(idx, B, shape, 3)
    pin, pout, pn = oracle.rulebook_subm(idx, shape, 3)
    worst = 0.0
    for exact in (False, True):
        d = (R32.draw32_exact if exact else R32.draw32)(rng, n, n, Cin, Cout, 3)
        sums = R.conv(d["x"], d["wp"], nbr)
        if exact:
            R32.assert_exactly_summable(sums)
        y = oracle.subm_conv(oracle.SparseTensor(d["x"], idx, shape, B), d["w"]).features
        for form in FORMS:
            V, e = _form(sums, d, form)
            worst = max(worst, R.assert_within(_oracle_form(oracle, y, d, form), V, ZERO(V) if exact else e, what=f"oracle forward {form}"))
        dx, dw = oracle.conv_backward(d["x"], d["w"], pin, pout, pn, d["dy"])
        sd, sw = R.dgrad(d["dy"], d["wp"], nbr, n), R.wgrad(d["x"], d["dy"], nbr)
        R.assert_within(dx, sd.S, ZERO(sd.S) if exact else R32.epilogue(sd)[1], what="oracle dx")
        R.assert_within(dw.reshape(Cout, 27, Cin).transpose(1, 0, 2), sw.S, ZERO(sw.S) if exact else R32.wgrad_bound(sw, 0), what="oracle dW")
        if not exact:
            # a 16-bit store of the first layer's result lies inside the 16-bit bound and outside the f32 bound
            want = _oracle_form(oracle, y, d, FORMS[2])
            for td in (torch.bfloat16, torch.float16):
                R.assert_within(torch.from_numpy(want).to(td), *_form(sums, d, FORMS[2], td), what="rounded")
                with pytest.raises(R.OutOfBound):
                    R.assert_within(torch.from_numpy(want).to(td), *_form(sums, d, FORMS[2]), what="16-bit against the f32 bound")
    assert 0.0 < worst <= 1.0
    print(f"worst err / bound of the oracle's forward {Cin}->{Cout}: {worst:.3g}")


@pytest.mark.parametrize("Cin,Cout", [(16, 32), (32, 64), (64, 128), (128, 128)])
@pytest.mark.parametrize("k,s,p", GEOMS)
def test_oracle_strided_inside_the_f32_bound_and_exact_on_integers(oracle, rng, k, s, p, Cin, Cout):
    B, shape, n = 2, [11, 16, 17], 1500
    idx = _random_sites(rng, B, shape, n)
    out, osh, nbr = R.neighbours_strided(idx, B, shape, k, s, p)
    o_idx, _, pin, pout, pn = oracle.rulebook_strided(idx, shape, k, s, p)
    m = R.match_rows(out, o_idx, osh)
    nbr = np.ascontiguousarray(nbr[:, m])             # in the oracle's row order
    K = nbr.shape[0]
    for exact in (False, True):
        d = (R32.draw32_exact if exact else R32.draw32)(rng, n, out.shape[0], Cin, Cout, k)
        sums = R.conv(d["x"], d["wp"], nbr)
        y = oracle.sparse_conv(oracle.SparseTensor(d["x"], idx, shape, B), d["w"], s, p)
        assert np.array_equal(y.indices, o_idx)
        for form in FORMS[:2]:
            V, e = _form(sums, d, form)
            R.assert_within(_oracle_form(oracle, y.features, d, form), V, ZERO(V) if exact else e, what=f"oracle strided forward {form}")
        dx, dw = oracle.conv_backward(d["x"], d["w"], pin, pout, pn, d["dy"])
        sd, sw = R.dgrad(d["dy"], d["wp"], nbr, n), R.wgrad(d["x"], d["dy"], nbr)
        R.assert_within(dx, sd.S, ZERO(sd.S) if exact else R32.epilogue(sd)[1], what="oracle dx")
        R.assert_within(dw.reshape(Cout, K, Cin).transpose(1, 0, 2), sw.S, ZERO(sw.S) if exact else R32.wgrad_bound(sw, 0), what="oracle dW")


@pytest.mark.parametrize("Cin,Cout", [(5, 16), (16, 32), (128, 128)])
def test_subset_helper_returns_the_bits_of_the_full_oracle_call(oracle, rng, Cin, Cout):
    B, shape, n = 2, [7, 16, 17], 1200
    idx = _random_sites(rng, B, shape, n)
    nbr = R.neighbours_subm(idx, B, shape, 3)
    d = R32.draw32(rng, n, n, Cin, Cout, 3)
    y = oracle.subm_conv(oracle.SparseTensor(d["x"], idx, shape, B), d["w"]).features
    rows = np.unique(np.concatenate([np.arange(16), np.arange(n - 16, n), rng.integers(0, n, 300)]))
    assert np.array_equal(R32.oracle_rows(oracle, d["x"], d["w"], nbr, rows), y[rows])
    want = oracle.scale_shift_act(y, d["sc"], d["sh"], d["res"], relu=True)
    assert np.array_equal(R32.oracle_rows(oracle, d["x"], d["w"], nbr, rows, d["sc"], d["sh"], d["res"], True), want[rows])
    assert np.array_equal(R32.oracle_rows(oracle, d["x"], d["w"], nbr, rows[::-1]), y[rows[::-1]]), "rows in any order"
    pin, pout, pn = R32.subset_pairs(nbr, rows)
    for k in range(27):
        assert (np.diff(pout[k, :pn[k]]) > 0).all() and (nbr[k, rows[pout[k, :pn[k]]]] == pin[k, :pn[k]]).all()
    assert int(pn.sum()) == int((nbr[:, rows] >= 0).sum())
    # strided table: the same through the oracle's own row order
    out, osh, nb2 = R.neighbours_strided(idx, B, shape, 3, 2, 1)
    if Cin >= 16:
        d = R32.draw32(rng, n, out.shape[0], Cin, Cout, 3)
        ys = oracle.sparse_conv(oracle.SparseTensor(d["x"], idx, shape, B), d["w"], 2, 1)
        m = R.match_rows(out, ys.indices, osh)        # oracle row -> reference row
        rows = rng.permutation(out.shape[0])[:200]
        assert np.array_equal(R32.oracle_rows(oracle, d["x"], d["w"], nb2[:, m], rows), ys.features[rows])


# ------------------------------------------------------------------------------------------------ planted defects: forward
def _sheet_sites(shape, n_min):
    rng = np.random.default_rng(1234)
    idx = _sheet(rng, 1, shape)
    idx = idx[np.lexsort((idx[:, 1], idx[:, 3], idx[:, 2], idx[:, 0]))]
    n = (idx.shape[0] - 16) // 16 * 16 + 5             # not a multiple of 16
    assert n > n_min, (n, n_min)
    return idx[:n], n


@pytest.mark.parametrize("C", [16, 64, 128])
def test_every_planted_forward_defect_is_rejected(oracle, C):
    """The honest result is the ORACLE's (the chain the kernels claim); every defect is rejected in every epilogue form, by the
    bound on random data and bit for bit on integer data.  The ranges are those of the restated split with a small grid, so that
    both regimes of wave_plan occur at a size the CPU affords: G = 3 (ranges of 2.3 tiles: the persistent loop) and a grid of
    5-block ranges (bpw = 2, one wave with nothing)."""
    rng = np.random.default_rng(1234)
    B, shape = 1, [5, 45, 45]
    tile = R32.tile_rows(C)
    idx, n = _sheet_sites(shape, 7 * tile)
    nbr = R.neighbours_subm(idx, B, shape, 3)
    G_full, G_bpw = 3, (n + 15) // 16 // 5
    rb, re = R32.ranges(n, G_full)
    assert not R32.wave_plan(int(rb[1]), int(re[1]), C)[0] and re[1] - rb[1] > 2 * tile
    sb, se = R32.ranges(n, G_bpw)
    small, bpw, plan = R32.wave_plan(int(sb[2]), int(se[2]), C)
    assert small and bpw == 2 and plan[3] == [] and len(plan[1]) == 1
    # a row in the second tile of range 1 with a neighbour at offset 14, and its block
    t1 = int(rb[1]) + tile
    r = next(r for r in range(t1 + 3, n - 1) if nbr[14, r] >= 0)
    k, blk = 14, r // 16 * 16
    live = np.arange(blk, blk + 16)[nbr[k, blk:blk + 16] >= 0]
    for exact in (False, True):
        d = (R32.draw32_exact if exact else R32.draw32)(rng, n, n, C, C, 3)
        sums = R.conv(d["x"], d["wp"], nbr)
        acc = torch.from_numpy(oracle.subm_conv(oracle.SparseTensor(d["x"], idx, shape, B), d["w"]).features)
        wt = np.ascontiguousarray(d["w"].reshape(C, 3, 3, 3, C // 16, 4, 4).swapaxes(5, 6).reshape(d["w"].shape))   # 4 x 4 transposed groups
        acc_t = torch.from_numpy(oracle.subm_conv(oracle.SparseTensor(d["x"], idx, shape, B), wt).features)
        x, wp = torch.from_numpy(d["x"]), torch.from_numpy(d["wp"])
        for form in FORMS:
            V, e = _form(sums, d, form)
            if exact:
                e = ZERO(V)
            ep = lambda a: torch.from_numpy(_oracle_form(oracle, a.numpy(), d, form))
            good = ep(acc)
            worst = R.assert_within(good, V, e, n, tile, "honest")
            assert worst <= 1.0 and (not exact or worst == 0.0)

            def rejected(out):
                with pytest.raises(R.OutOfBound) as ei:
                    R.assert_within(out, V, e, n, tile, "planted")
                return str(ei.value)

            # a (row, offset) pair dropped
            a = acc.clone()
            a[r] -= x[nbr[k, r]] @ wp[k].T
            msg = rejected(ep(a))
            assert msg.startswith("planted: 1 of") and f"first rows [{r}]" in msg
            # one 16-channel input chunk of one offset dropped for a 16-row block
            a = acc.clone()
            a[live] -= x[torch.from_numpy(nbr[k, live])][:, -16:] @ wp[k][:, -16:].T
            rejected(ep(a))
            # the 4 x 4 transposition of the 16-channel groups applied to the weights only
            rejected(ep(acc_t))
            # the clamped last row of a range written into the first row of the next range
            o = good.clone()
            o[int(rb[2])] = good[int(re[1]) - 1]
            assert rejected(o).startswith("planted: 1 of")
            # one wave's blocks left at the prefill in the bpw regime
            for fill in (float("nan"), 0.0):
                o = good.clone()
                o[plan[1][0][0]:plan[1][0][1]] = fill
                assert rejected(o).startswith("planted: 32 of")
            # one full tile of a range written to the next tile's rows
            o = good.clone()
            o[t1:t1 + tile] = good[t1 - tile:t1]
            rejected(o)
            # two rows swapped by a perm that is still a permutation
            o = good.clone()
            o[[blk + 3, blk + 11]] = good[[blk + 11, blk + 3]]
            assert rejected(o).startswith("planted: 2 of")
            # the rows behind the last multiple of 16 left at the prefill
            o = good.clone()
            o[n // 16 * 16:] = float("nan")
            assert f"{n % 16} of" in rejected(o)


def test_first_layer_rows_of_the_second_round_left_at_the_prefill_are_rejected(oracle):
    """spconv_first_kernel (5 -> 16): rows from 524 288 on — its second grid-stride round — left at the prefill, in f32 and with the
    16-bit store of conv_input under the 16-bit engines (the integer result rounded once: exact16)"""
    rng = np.random.default_rng(1234)
    B, shape = 9, [5, 200, 200]
    idx = _sheet(rng, B, shape)
    idx = idx[np.lexsort((idx[:, 1], idx[:, 3], idx[:, 2], idx[:, 0]))]
    n = R32.FIRST_ROUND_ROWS + 3005
    assert idx.shape[0] >= n
    idx = idx[:n]
    nbr = R.neighbours_subm(idx, B, shape, 3)
    for exact in (False, True):
        d = (R32.draw32_exact if exact else R32.draw32)(rng, n, n, 5, 16, 3)
        sums = R.conv(d["x"], d["wp"], nbr)
        y = oracle.subm_conv(oracle.SparseTensor(d["x"], idx, shape, B), d["w"]).features
        good = torch.from_numpy(_oracle_form(oracle, y, d, FORMS[2]))
        for td in (torch.float32, torch.bfloat16, torch.float16):
            V, e = _form(sums, d, FORMS[2], td)
            if exact:
                V, e = R32.exact16(V, td).double(), ZERO(V)
            assert R.assert_within(good.to(td), V, e, n, 256, "honest") <= 1.0
            o = good.to(td).clone()
            o[R32.FIRST_ROUND_ROWS:] = float("nan") if td == torch.float32 else 0.0     # (a NaN prefill, or whatever lay there)
            with pytest.raises(R.OutOfBound) as ei:
                R.assert_within(o, V, e, n, 256, "planted")
            assert f"first rows [{R32.FIRST_ROUND_ROWS}," in str(ei.value)
    # and the chain check sees it on its own rows
    rows = R32.rows_around(n, [R32.FIRST_ROUND_ROWS], rng)
    assert {R32.FIRST_ROUND_ROWS - 1, R32.FIRST_ROUND_ROWS, n - 1} <= set(rows.tolist())
    assert np.array_equal(R32.oracle_rows(oracle, d["x"], d["w"], nbr, rows, d["sc"], d["sh"], d["res"], True), good.numpy()[rows])


def test_planted_defects_of_the_class_sort_are_rejected(rng):
    B, shape = 1, [5, 60, 60]
    idx, n = _sheet_sites(shape, 4000)
    cls = R32.zclass(R.neighbours_subm(idx, B, shape, 3))
    assert set(np.unique(cls).tolist()) == {0, 1, 2, 3} or len(np.unique(cls)) >= 3
    G = 13
    rb, re = R32.ranges(n, G)
    perm = np.concatenate([b + np.argsort(cls[b:e], kind="stable") for b, e in zip(rb, re)])
    R32.check_perm(perm, cls, n, G)
    b, e = int(rb[5]), int(re[5])

    def rejected(p, words):
        with pytest.raises(AssertionError, match=words):
            R32.check_perm(p, cls, n, G)

    p = perm.copy(); p[b] = perm[b + 1]
    rejected(p, "not a permutation")
    p = perm.copy(); p[[e - 1, e]] = perm[[e, e - 1]]
    rejected(p, "out of its workgroup range")
    j = b + int(np.nonzero(np.diff(cls[perm[b:e]]) > 0)[0][0])           # the last row of a class and the first of the next
    p = perm.copy(); p[[j, j + 1]] = perm[[j + 1, j]]
    rejected(p, "a class descends")
    j = b + int(np.nonzero(np.diff(cls[perm[b:e]]) == 0)[0][0])
    p = perm.copy(); p[[j, j + 1]] = perm[[j + 1, j]]
    rejected(p, "do not keep their order")
    rejected(np.arange(n), "a class descends")                           # (row order where the ranges are short enough to sort)
    rejected(np.concatenate([perm[:-1], [n]]), "outside the rows")
    # the whole tensor sorted at once: classes in order, stable — and rows outside their ranges
    rejected(np.argsort(cls, kind="stable"), "out of its workgroup range")
    # a range of more than 16 384 rows keeps its own order
    big = 40000
    c2 = np.resize(cls, big)
    R32.check_perm(np.arange(big), c2, big, 2)
    with pytest.raises(AssertionError, match="too long to sort"):
        R32.check_perm(np.concatenate([np.argsort(c2[:20000], kind="stable"), np.arange(20000, big)]), c2, big, 2)


# ------------------------------------------------------------------------------------------------ planted defects: weight gradient
@pytest.mark.parametrize("Cin,Cout", [(5, 16), (16, 16), (64, 64), (64, 128)])
def test_planted_wgrad_defects_are_rejected(Cin, Cout):
    """An emulation of the two-stage weight gradient (f32 partial sums over the device's chunks of the n rows, added in chunk
    order) and what a wrong one would give: the last chunk dropped, the chunk borders mixed from the capacity and from n (rows
    counted twice), the rows between r1 and the end of its 16-row tile included, the module layout transposed.  At these few
    thousand pairs per offset the rounding bound sees all of them; at the 10^5 pairs of the GPU cases it is wider than a chunk's
    tail, which is why every defect must ALSO be rejected bit for bit on integer inputs."""
    rng = np.random.default_rng(1234)
    B, shape = 1, [5, 50, 50]
    idx_all = _sheet(rng, B, shape)
    idx_all = idx_all[np.lexsort((idx_all[:, 1], idx_all[:, 3], idx_all[:, 2], idx_all[:, 0]))]
    cap = idx_all.shape[0]
    chunks = 3
    n = chunks * (128 * 8 + 1) + 5                     # 3080: the device's chunks are 1152 rows, the last one short
    assert cap > n + 16 and n % 16
    rpc_dev, rpc_host = R32.wgrad_rows_per_chunk(n, chunks), R32.wgrad_rows_per_chunk(cap, chunks)
    assert rpc_dev == 1152 and rpc_host > rpc_dev
    nbr = R.neighbours_subm(idx_all[:n], B, shape, 3)
    nbr_all = R.neighbours_subm(idx_all, B, shape, 3)   # (what lies in the table behind n: rows a wrong kernel would read)
    assert np.array_equal(nbr_all[13], np.arange(cap))
    P = chunks

    def f32_wgrad(x, dy, defect=None):
        x, dy = torch.from_numpy(x), torch.from_numpy(dy)
        dw = torch.zeros((27, Cout, Cin), dtype=torch.float32)
        for c in range(chunks):
            r0 = min(n, c * rpc_dev)
            r1 = min(n, r0 + (rpc_host if defect == "borders from cap" else rpc_dev))
            table = nbr
            if defect == "last chunk dropped" and c == chunks - 1:
                continue
            if defect == "tile tail":
                r1, table = r0 + (r1 - r0 + 15) // 16 * 16, nbr_all
            for k in range(27):
                o = r0 + np.nonzero(table[k, r0:r1] >= 0)[0]
                dw[k] += dy[torch.from_numpy(o)].T @ x[torch.from_numpy(table[k][o])]
        return dw

    for exact in (False, True):
        d = (R32.draw32_exact if exact else R32.draw32)(rng, cap, cap, Cin, Cout, 3)
        sums = R.wgrad(d["x"][:n], d["dy"][:n], nbr)
        V, e = sums.S, ZERO(sums.S) if exact else R32.wgrad_bound(sums, P)
        good = f32_wgrad(d["x"], d["dy"])
        worst = R.assert_within(good, V, e, what="honest dW")
        assert worst < 0.1 and (not exact or worst == 0.0)
        for defect in ("last chunk dropped", "borders from cap", "tile tail"):
            with pytest.raises(R.OutOfBound):
                R.assert_within(f32_wgrad(d["x"], d["dy"], defect), V, e, what=defect)
        # asked for the module's (Cout, K, Cin), written as (K, Cout, Cin)
        module = lambda buf: buf.reshape(Cout, 27, Cin).permute(1, 0, 2)      # how the GPU file reads a module_shape result
        R.assert_within(module(good.permute(1, 0, 2).contiguous()), V, e, what="honest module layout")
        with pytest.raises(R.OutOfBound):
            R.assert_within(module(good), V, e, what="module layout transposed")
