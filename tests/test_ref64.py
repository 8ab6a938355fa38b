"""tests/ref64.py, the float64 reference of the at-scale GPU tests (tests/test_gpu_conv_at_scale.py), checked on the CPU:
against the C oracle (itself pinned to torch's dense conv3d by tests/test_oracle_spconv.py), whose f32 results must lie inside
the derived bound and whose rulebooks must name the same pairs; and against PLANTED DEFECTS — what a subtly wrong kernel would
write, applied to a correct f32 result — every one of which the comparator must reject, with inputs drawn as in the GPU tests."""
import numpy as np
import pytest
import torch

import ref64 as R
from test_gpu_rows128 import _sheet

PAIRS = [(16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128)]
GEOMS = [(3, 2, 1), (3, 2, (0, 1, 1)), ((3, 1, 1), (2, 1, 1), 0)]      # (k, s, p) of the backbone's strided layers


def _random_sites(rng, B, shape, n):
    cells = B * shape[0] * shape[1] * shape[2]
    lin = rng.choice(cells, size=n, replace=False)
    b, rem = np.divmod(lin, shape[0] * shape[1] * shape[2])
    z, rem = np.divmod(rem, shape[1] * shape[2])
    y, x = np.divmod(rem, shape[2])
    return np.stack([b, z, y, x], 1).astype(np.int32)


def _oracle_pairs(pin, pout, pn):
    s = set()
    for k in range(pin.shape[0]):
        s |= set(zip([k] * int(pn[k]), pin[k, :pn[k]].tolist(), pout[k, :pn[k]].tolist()))
    return s


def test_subm_neighbours_equal_the_oracle_rulebook(oracle, rng):
    B, shape = 3, [7, 20, 21]
    idx = _random_sites(rng, B, shape, 2500)
    nbr = R.neighbours_subm(idx, B, shape, 3)
    assert R.pairs_of(nbr) == _oracle_pairs(*oracle.rulebook_subm(idx, shape, 3))
    assert (nbr[13] == np.arange(idx.shape[0])).all()


@pytest.mark.parametrize("k,s,p", GEOMS)
def test_strided_neighbours_equal_the_oracle_rulebook(oracle, rng, k, s, p):
    B, shape = 2, [11, 20, 23]
    idx = _random_sites(rng, B, shape, 1500)
    out, osh, nbr = R.neighbours_strided(idx, B, shape, k, s, p)
    o_idx, o_shape, pin, pout, pn = oracle.rulebook_strided(idx, shape, k, s, p)
    assert osh == o_shape and out.shape[0] == o_idx.shape[0]
    m = R.match_rows(out, o_idx, osh)                # oracle row -> reference row
    assert np.array_equal(out[m], o_idx)
    want = {(kk, i, int(m[o])) for kk, i, o in _oracle_pairs(pin, pout, pn)}
    assert R.pairs_of(nbr) == want


@pytest.mark.parametrize("td", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Cin,Cout", PAIRS)
def test_oracle_subm_forward_and_backward_inside_the_bound(oracle, rng, Cin, Cout, td):
    B, shape, n = 2, [7, 16, 17], 1200
    idx = _random_sites(rng, B, shape, n)
    d = R.draw(rng, n, n, Cin, Cout, 3, td)
    nbr = R.neighbours_subm(idx, B, shape, 3)
    sums = R.conv(d["x"], d["wp"], nbr)
    y = oracle.subm_conv(oracle.SparseTensor(d["x"], idx, shape, B), d["w"]).features
    worst = R.assert_within(y, *R.epilogue(sums), what="oracle.subm_conv")
    want = oracle.scale_shift_act(y, d["sc"], d["sh"], d["res"], relu=True)
    worst = max(worst, R.assert_within(want, *R.epilogue(sums, d["sc"], d["sh"], d["res"], True), what="oracle.scale_shift_act"))
    assert worst < 1.0
    # a result rounded to the 16-bit type lies inside the 16-bit bound, and a 16-bit result is OUTSIDE the f32 bound somewhere
    V, e16 = R.epilogue(sums, d["sc"], d["sh"], d["res"], True, out_dtype=td)
    R.assert_within(torch.from_numpy(want).to(td), V, e16, what="rounded")
    with pytest.raises(R.OutOfBound):
        R.assert_within(torch.from_numpy(want).to(td), *R.epilogue(sums, d["sc"], d["sh"], d["res"], True), what="16-bit against the f32 bound")
    pin, pout, pn = oracle.rulebook_subm(idx, shape, 3)
    dx, dw = oracle.conv_backward(d["x"], d["w"], pin, pout, pn, d["dy"])
    R.assert_within(dx, *R.epilogue(R.dgrad(d["dy"], d["wp"], nbr, n)), what="oracle dx")
    dw_packed = dw.reshape(Cout, 27, Cin).transpose(1, 0, 2)
    R.assert_within(dw_packed, *R.epilogue(R.wgrad(d["x"], d["dy"], nbr)), what="oracle dW")


@pytest.mark.parametrize("Cin,Cout", [(16, 32), (32, 64), (64, 128), (128, 128)])
@pytest.mark.parametrize("k,s,p", GEOMS)
def test_oracle_strided_forward_and_backward_inside_the_bound(oracle, rng, k, s, p, Cin, Cout):
    td = torch.bfloat16
    B, shape, n = 2, [11, 16, 17], 1500
    idx = _random_sites(rng, B, shape, n)
    out, osh, nbr = R.neighbours_strided(idx, B, shape, k, s, p)
    m_out = out.shape[0]
    d = R.draw(rng, n, m_out, Cin, Cout, k, td)
    y = oracle.sparse_conv(oracle.SparseTensor(d["x"], idx, shape, B), d["w"], s, p)
    m = R.match_rows(out, y.indices, osh)
    sums = R.conv(d["x"], d["wp"], nbr[:, m])        # in the oracle's row order
    R.assert_within(y.features, *R.epilogue(sums), what="oracle.sparse_conv")
    R.assert_within(oracle.scale_shift_act(y.features, d["sc"], d["sh"], None, relu=True), *R.epilogue(sums, d["sc"], d["sh"], None, True),
                    what="oracle.scale_shift_act")
    o_idx, _, pin, pout, pn = oracle.rulebook_strided(idx, shape, k, s, p)
    assert np.array_equal(o_idx, y.indices)
    dx, dw = oracle.conv_backward(d["x"], d["w"], pin, pout, pn, d["dy"])
    R.assert_within(dx, *R.epilogue(R.dgrad(d["dy"], d["wp"], nbr[:, m], n)), what="oracle dx")
    K = nbr.shape[0]
    R.assert_within(dw.reshape(Cout, K, Cin).transpose(1, 0, 2), *R.epilogue(R.wgrad(d["x"], d["dy"], nbr[:, m])), what="oracle dW")


# ------------------------------------------------------------------------------------------------ planted defects
def _f32_forward(d, nbr, form, order):
    """a CORRECT f32 result: f32 products summed offset by offset in `order`, the f32 epilogue, as a kernel would"""
    x, wp = torch.from_numpy(d["x"]), torch.from_numpy(d["wp"])
    acc = torch.zeros((nbr.shape[1], wp.shape[1]), dtype=torch.float32)
    for k in order:
        o = torch.from_numpy(np.nonzero(nbr[k] >= 0)[0])
        acc.index_add_(0, o, x[torch.from_numpy(nbr[k][o.numpy()])] @ wp[k].T)
    return acc, _f32_epilogue(acc, d, form)


def _f32_epilogue(acc, d, form):
    res, scaled, relu = form
    v = acc.clone()
    if scaled:
        v = v * torch.from_numpy(d["sc"]) + torch.from_numpy(d["sh"])
    if res:
        v = v + torch.from_numpy(d["res"])
    return v.clamp_min(0) if relu else v


FORMS = [(False, False, False), (False, True, True), (True, True, True), (True, False, False)]   # (residual, scale / shift, relu)


def _ref_form(sums, d, form, out_dtype):
    res, scaled, relu = form
    return R.epilogue(sums, d["sc"] if scaled else None, d["sh"] if scaled else None, d["res"] if res else None, relu, out_dtype)


@pytest.mark.parametrize("td", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("C,tile", [(16, 128), (64, 256), (128, 384)])
def test_every_planted_forward_defect_is_rejected(C, tile, td):
    """Sites, inputs and epilogue forms of the GPU tests (the sheet of test_gpu_rows128.py), the output stored in the 16-bit
    type: the widest bound a GPU case is held to.  The honest result passes far inside; every defect is rejected in every form."""
    rng = np.random.default_rng(1234)
    B, shape = 1, [5, 60, 60]
    idx = _sheet(rng, B, shape)
    idx = idx[np.lexsort((idx[:, 1], idx[:, 3], idx[:, 2], idx[:, 0]))]
    n = (idx.shape[0] - 16) // 16 * 16 + 5             # not a multiple of 16
    idx = idx[:n]
    assert n > 2 * tile + 16
    nbr = R.neighbours_subm(idx, B, shape, 3)
    d = R.draw(rng, n, n, C, C, 3, td)
    sums = R.conv(d["x"], d["wp"], nbr)
    x, wp, res = torch.from_numpy(d["x"]), torch.from_numpy(d["wp"]), torch.from_numpy(d["res"])
    # a row in the second tile with a neighbour at an offset that is not the centre, whose next row exists
    r = next(r for r in range(tile + 3, n - 1) if nbr[14, r] >= 0 and nbr[14, r] + 1 < n)
    k, blk = 14, r // 16 * 16
    rows = torch.arange(blk, blk + 16)
    for form in FORMS:
        V, e = _ref_form(sums, d, form, td)
        store = lambda v: v.to(td)
        acc, good = _f32_forward(d, nbr, form, range(26, -1, -1))
        worst = R.assert_within(store(good), V, e, n, tile, "honest")
        assert worst <= 1.0
        worst32 = R.assert_within(good, *_ref_form(sums, d, form, torch.float32), n, tile, "honest f32")
        assert worst32 < 0.05, worst32

        def rejected(acc_bad=None, out_bad=None, dd=d):
            out = out_bad if out_bad is not None else store(_f32_epilogue(acc_bad, dd, form))
            with pytest.raises(R.OutOfBound) as ei:
                R.assert_within(out, V, e, n, tile, "planted")
            return str(ei.value)

        # one (row, offset) pair dropped
        a = acc.clone()
        a[r] -= x[nbr[k, r]] @ wp[k].T
        msg = rejected(a)
        assert msg.startswith("planted: 1 of") and f"first rows [{r}]" in msg
        # the last 32-channel K step of one offset dropped for one 16-row block (16-channel layers: the upper half of a step)
        a = acc.clone()
        kc = min(32, C // 2) if C == 16 else 32
        live = rows[torch.from_numpy(nbr[k, blk:blk + 16] >= 0)]
        a[live] -= x[torch.from_numpy(nbr[k, live.numpy()])][:, -kc:] @ wp[k][:, -kc:].T
        rejected(a)
        # a row's neighbour taken from row + 1
        a = acc.clone()
        a[r] += (x[nbr[k, r] + 1] - x[nbr[k, r]]) @ wp[k].T
        rejected(a)
        # one round's tile written to the rows of the next
        o = store(good).clone()
        o[tile:2 * tile] = store(good)[0:tile]
        rejected(out_bad=o)
        # the rows behind the last multiple of 16 left at the output's prefill (NaN where the call takes `out=`, else whatever)
        for fill in (float("nan"), 0.0):
            o = store(good).clone()
            o[n // 16 * 16:] = fill
            msg = rejected(out_bad=o)
            assert f"{n % 16} of" in msg
        # residual rows of two positions of a block swapped
        if form[0]:
            sw = dict(d)
            sw["res"] = d["res"].copy()
            sw["res"][[blk + 3, blk + 11]] = d["res"][[blk + 11, blk + 3]]
            msg = rejected(acc, dd=sw)
            assert msg.startswith("planted: 2 of")
    assert torch.equal(res, torch.from_numpy(d["res"]))


@pytest.mark.parametrize("td", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Cin,Cout", [(16, 16), (64, 64), (64, 128)])
def test_planted_wgrad_defect_is_rejected(Cin, Cout, td):
    """The pairs behind the last multiple of 128 of an offset's pair list (the weight-gradient kernels cut the lists into chunks
    of multiples of 128 rows) left out.  gamma grows with the pairs T of an offset, so m lost pairs of T stand out of the bound
    only while m is not small against T^2 * 2^-23: a few thousand pairs per offset here; at the hundreds of thousands of the GPU
    cases the bound is wider than a lost tail, which is why those also run the integer inputs of draw_exact (no rounding at
    all: bound zero)."""
    rng = np.random.default_rng(1234)
    B, shape = 1, [5, 50, 50]
    idx = _sheet(rng, B, shape)
    idx = idx[np.lexsort((idx[:, 1], idx[:, 3], idx[:, 2], idx[:, 0]))]
    n = idx.shape[0]
    nbr = R.neighbours_subm(idx, B, shape, 3)
    d = R.draw(rng, n, n, Cin, Cout, 3, td)
    V, e = R.epilogue(R.wgrad(d["x"], d["dy"], nbr))
    x, dy = torch.from_numpy(d["x"]), torch.from_numpy(d["dy"])

    def f32_wgrad(drop_tail):
        dw = torch.zeros((27, Cout, Cin), dtype=torch.float32)
        for k in range(27):
            o = np.nonzero(nbr[k] >= 0)[0]
            if drop_tail:
                o = o[:o.shape[0] // 128 * 128]
            for c in range(0, o.shape[0], 128):          # chunk partials, then their sum: the two-stage order
                oc = o[c:c + 128]
                dw[k] += dy[torch.from_numpy(oc)].T @ x[torch.from_numpy(nbr[k][oc])]
        return dw

    assert R.assert_within(f32_wgrad(False), V, e, what="honest dW") < 0.05
    with pytest.raises(R.OutOfBound):
        R.assert_within(f32_wgrad(True), V, e, what="planted dW")
    # the integer inputs: every partial sum is an integer below 2^24, so f32 adds exactly in any order — bound zero
    dz = R.draw_exact(rng, n, n, Cin, Cout, td)
    sums = R.wgrad(dz["x"], dz["dy"], nbr)
    assert float(sums.A.max()) < 2 ** 24
    x, dy = torch.from_numpy(dz["x"]), torch.from_numpy(dz["dy"])
    zero = torch.zeros_like(sums.S)
    assert R.assert_within(f32_wgrad(False), sums.S, zero, what="exact dW") == 0.0
    with pytest.raises(R.OutOfBound):
        R.assert_within(f32_wgrad(True), sums.S, zero, what="planted exact dW")


def test_comparator_reports_blocks_and_rejects_nan():
    V = torch.zeros((800, 4), dtype=torch.float64)
    e = torch.full((800, 4), 1e-3, dtype=torch.float64)
    got = torch.zeros((800, 4))
    assert R.assert_within(got, V, e, 790, 384) == 0.0
    got[795] = float("nan")
    assert R.assert_within(got, V, e, 790, 384) == 0.0          # rows at and behind n are not looked at
    got[400:416] = 1.0
    got[3, 2] = float("nan")
    worst, rep = R.check(got, V, e, 790, 384)
    assert worst == float("inf") and "17 of 790 rows" in rep and "NaN elements: 1" in rep
    assert "16-row block within the 384-row tile: [1, 16, 0" in rep
