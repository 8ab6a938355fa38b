"""tests/train_trace.py must reject what it exists for.  One SubM 32 -> 32 layer, one strided 16 -> 32 layer and the zero-padded
5 -> 16 layer are EMULATED with torch on the CPU (f32 accumulation of 16-bit operands, a few thousand sheet sites, bf16 and fp16);
honest records pass with the worst ratio far below 1, and each planted defect is rejected and reported with the layer and the
quantity (out, dx or dw) at fault.  The recorder is run around a CPU stand-in Function whose input also feeds a residual branch:
what it catches is that call's own data gradient."""
import copy

import numpy as np
import pytest
import torch

import ref64 as R
import train_trace as TT
from test_gpu_rows128 import _sheet

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
B, SHAPE = 1, [5, 40, 40]


def _sites():
    idx = _sheet(np.random.default_rng(11), B, SHAPE)
    assert 2000 < idx.shape[0] < 4000
    return idx


def _acc32(x, wp, nbr):
    """sum_k x[nbr[k]] @ wp[k]^T accumulated in f32: what a kernel with exact products and an f32 accumulator computes"""
    out = torch.zeros((nbr.shape[1], wp.shape[1]), dtype=torch.float32)
    for k in range(nbr.shape[0]):
        o = np.nonzero(nbr[k] >= 0)[0]
        if o.shape[0]:
            out.index_add_(0, torch.from_numpy(o), x[torch.from_numpy(np.ascontiguousarray(nbr[k][o]))] @ wp[k].T)
    return out


def _wgrad32(x, g, nbr):
    dw = torch.zeros((nbr.shape[0], g.shape[1], x.shape[1]), dtype=torch.float32)
    for k in range(nbr.shape[0]):
        o = np.nonzero(nbr[k] >= 0)[0]
        if o.shape[0]:
            dw[k] = g[torch.from_numpy(o)].T @ x[torch.from_numpy(np.ascontiguousarray(nbr[k][o]))]
    return dw


def _module_layout(dw, ksize):
    K, Cout, Cin = dw.shape
    return np.ascontiguousarray(dw.permute(1, 0, 2).reshape(Cout, *ksize, Cin).numpy())


class Emulated:
    """an honest record of one layer and the pieces the planted defects are made of"""

    def __init__(self, name, td, subm, cin, cout, exact=False, pad_to=None, seed=3):
        rng = np.random.default_rng(seed)
        idx = _sites()
        self.td, self.subm, self.ksize = td, subm, [3, 3, 3]
        n_in = idx.shape[0]
        if subm:
            nbr, out_idx, osh, stride, padding = R.neighbours_subm(idx, B, SHAPE), idx, SHAPE, [1, 1, 1], [1, 1, 1]
        else:
            stride, padding = [2, 2, 2], [1, 1, 1]
            out_idx, osh, nbr = R.neighbours_strided(idx, B, SHAPE, 3, 2, 1)
            p = rng.permutation(out_idx.shape[0])          # the device's output rows are in an order of their own
            out_idx, nbr = out_idx[p], np.ascontiguousarray(nbr[:, p])
        n_out = nbr.shape[1]
        self.nbr, self.n_in, self.n_out = nbr, n_in, n_out
        if exact:
            z = R.draw_exact(rng, n_in, n_out, cin, cout, td)
            x, go = z["x"], z["dy"]
            w = rng.integers(-2, 3, (cout, 3, 3, 3, cin)).astype(np.float32)
        else:
            d = R.draw(rng, n_in, n_out, cin, cout, 3, td)
            x = d["x"]
            w = (rng.standard_normal((cout, 3, 3, 3, cin)) * 0.05).astype(np.float32)     # the f32 parameter: rounded by the function
            go = rng.standard_normal((n_out, cout)).astype(np.float32)                    # arrives in f32: rounded by the function
        self.cin_module = cin
        if pad_to:
            x = np.concatenate([x, np.zeros((n_in, pad_to - cin), np.float32)], 1)
            w = np.concatenate([w, np.zeros((cout, 3, 3, 3, pad_to - cin), np.float32)], 4)
            cin = pad_to
        self.x, self.w, self.go = torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(go)
        self.g = self.go.to(td).float()
        self.wp = self.packed(self.w)
        self.nbr_t = R.transpose_nbr(nbr, n_in)
        out = _acc32(self.x, self.wp, nbr).to(td).float()
        dx = _acc32(self.g, self.wp.transpose(1, 2).contiguous(), self.nbr_t).to(td).float()
        self.dw_packed = _wgrad32(self.x, self.g, nbr)
        dw = _module_layout(self.dw_packed, self.ksize)[..., :self.cin_module]
        self.rec = TT.Record(name=name, subm=subm, ksize=self.ksize, stride=stride, padding=padding, batch=B, in_shape=SHAPE, out_shape=list(osh),
                             in_idx=idx, out_idx=out_idx, dtype=td, x=x, w=w, out=out.numpy(), go=go, dx=dx.numpy(), dw=dw, n_in=n_in, n_out=n_out,
                             cap_out=n_out, rows=n_out, ranked=False, prepacked=True)

    def packed(self, w):
        Cout, Cin = w.shape[0], w.shape[-1]
        return w.to(self.td).float().reshape(Cout, 27, Cin).permute(1, 0, 2).contiguous()

    def with_(self, **kw):
        r = copy.copy(self.rec)
        r.__dict__.update(kw)
        return r

    def dx_from(self, slabs, table=None):
        """the data gradient the forward kernel gives on `slabs` (K, Cin, Cout) and `table`"""
        return _acc32(self.g, slabs, self.nbr_t if table is None else table).to(self.td).float().numpy()


_CACHE = {}


def layer(kind, td, exact=False):
    k = (kind, td, exact)
    if k not in _CACHE:
        _CACHE[k] = (Emulated("subm 32->32", td, True, 32, 32, exact) if kind == "subm" else
                     Emulated("strided 16->32", td, False, 16, 32, exact) if kind == "strided" else
                     Emulated("padded 5->16", td, True, 5, 16, exact, pad_to=16))
    return _CACHE[k]


def _rejected(rec, quantity, exact=False):
    r = TT.check_layer(rec, exact=exact)
    assert r.fails, f"{rec.name}: a wrong {quantity} passed, ratios {r.ratio}"
    assert all(f.startswith(f"{rec.name}: {quantity}: ") for f in r.fails), r.fails      # the layer and the quantity at fault, and no other
    assert r.ratio[quantity] > 1.0
    print(f"REJECTED {rec.name} | {quantity} | {r.fails[0].splitlines()[0]}")
    return r


@pytest.mark.parametrize("td", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["subm", "strided", "padded"])
def test_honest_records_pass_far_inside_the_bound(kind, td, capsys):
    L = layer(kind, td)
    results, fails = TT.check_step(f"emulated {td}", [L.rec])
    assert not fails, "\n".join(fails)
    r = results[0]
    assert set(r.ratio) == {"out", "dx", "dw"}
    # a 16-bit output's ratio is that of its final rounding, at most the half ulp the bound grants; the f32 weight gradient shows
    # the accumulation: far below 1
    assert r.ratio["out"] < 1.0 and r.ratio["dx"] < 1.0 and r.ratio["dw"] < 0.2, r.ratio
    assert r.min_share >= 0.2, r.min_share                     # every offset is live: no defect hides behind the centre offset
    assert L.rec.dw.shape[-1] == L.cin_module
    assert "RATIO emulated" in capsys.readouterr().out


@pytest.mark.parametrize("td", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["subm", "strided"])
def test_integer_records_are_exact(kind, td):
    L = layer(kind, td, exact=True)
    r = TT.check_layer(L.rec, exact=True)
    assert not r.fails and max(r.ratio.values()) == 0.0, (r.fails, r.ratio)


@pytest.mark.parametrize("td", DTYPES, ids=IDS)
def test_dx_from_slabs_transposed_but_not_mirrored(td):
    L = layer("subm", td)
    mirrored = L.wp.flip(0).transpose(1, 2).contiguous()
    # (the honest form first: the forward's own table with mirrored and transposed slabs IS the data gradient)
    assert not TT.check_layer(L.with_(dx=L.dx_from(mirrored, L.nbr))).fails
    _rejected(L.with_(dx=L.dx_from(L.wp.transpose(1, 2).contiguous(), L.nbr)), "dx")


@pytest.mark.parametrize("td", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["subm", "strided"])
def test_dx_with_two_offsets_slabs_exchanged(kind, td):
    L = layer(kind, td)
    slabs = L.wp.transpose(1, 2).contiguous()
    slabs[[3, 17]] = slabs[[17, 3]]
    _rejected(L.with_(dx=L.dx_from(slabs)), "dx")


@pytest.mark.parametrize("td", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["subm", "strided"])
def test_dx_missing_one_neighbour_of_one_row(kind, td):
    L = layer(kind, td)
    table = L.nbr_t.copy()
    k = 5
    i = int(np.nonzero(table[k] >= 0)[0][7])
    table[k, i] = -1
    r = _rejected(L.with_(dx=L.dx_from(L.wp.transpose(1, 2).contiguous(), table)), "dx")
    assert f"first rows [{i}]" in r.fails[0]


@pytest.mark.parametrize("td", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["subm", "strided"])
def test_dw_missing_the_last_pair_of_one_offset(kind, td):
    """the integer form, where the bound is zero: at a rounding bound one pair of thousands would hide"""
    L = layer(kind, td, exact=True)
    k = 20
    o = int(np.nonzero(L.nbr[k] >= 0)[0][-1])
    dw = L.dw_packed.clone()
    lost = torch.outer(L.g[o], L.x[L.nbr[k, o]])
    assert float(lost.abs().max()) > 0
    dw[k] -= lost
    _rejected(L.with_(dw=_module_layout(dw, L.ksize)), "dw", exact=True)


@pytest.mark.parametrize("td", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["subm", "strided"])
def test_dw_of_one_offset_written_at_its_mirror(kind, td):
    L = layer(kind, td)
    dw = L.dw_packed.clone()
    dw[26 - 4] = L.dw_packed[4]
    _rejected(L.with_(dw=_module_layout(dw, L.ksize)), "dw")


@pytest.mark.parametrize("td", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["subm", "strided"])
def test_out_from_a_weight_one_update_older(kind, td):
    """a stale prepack: the slabs of the weight before the optimizer's last step (1e-3 per element, Adam's first steps at lr 1e-3)"""
    L = layer(kind, td)
    rng = np.random.default_rng(8)
    older = L.w - 1e-3 * torch.from_numpy(np.sign(rng.standard_normal(tuple(L.w.shape))).astype(np.float32))
    out = _acc32(L.x, L.packed(older), L.nbr).to(td).float().numpy()
    _rejected(L.with_(out=out), "out")


@pytest.mark.parametrize("td", DTYPES, ids=IDS)
def test_padded_gradient_sliced_at_the_wrong_end(td):
    L = layer("padded", td)
    full = _module_layout(L.dw_packed, L.ksize)
    assert full.shape[-1] == 16 and not full[..., 5:].any()         # (the padding's channels see zeros only)
    _rejected(L.with_(dw=np.ascontiguousarray(full[..., -5:])), "dw")
    r = TT.check_layer(L.with_(dw=full))                             # the padded shape is not the module's
    assert not r.fails, r.fails
    r = TT.check_layer(L.with_(dw=np.ascontiguousarray(full[:8, ..., :5])))
    assert r.fails and r.fails[0].startswith("padded 5->16: dw: weight.grad has shape")


def test_subnormal_operands_widen_the_bound_by_their_terms_only():
    """fp16 gradients with subnormals: a kernel that flushes them stays inside the widened bound, one that loses a NORMAL term of
    the same row does not"""
    td = torch.float16
    L = layer("subm", td)
    go = L.go.clone()
    go[::3] *= 2.0 ** -15                                            # a third of the rows: subnormal in fp16 after rounding
    g = go.to(td).float()
    sub = (g != 0) & (g.abs() < 2.0 ** -14)
    assert 0.2 < float(sub.float().mean()) < 0.4
    slabs = L.wp.transpose(1, 2).contiguous()
    keep = _acc32(g, slabs, L.nbr_t).to(td).float().numpy()
    flush = _acc32(g * ~sub, slabs, L.nbr_t).to(td).float().numpy()
    dw = lambda gg: _module_layout(_wgrad32(L.x, gg, L.nbr), L.ksize)
    for dx, w in ((keep, dw(g)), (flush, dw(g * ~sub))):
        r = TT.check_layer(L.with_(go=go.numpy(), dx=dx, dw=w))
        assert not r.fails, r.fails
        assert 0.2 < r.sub["go"] < 0.4 and r.sub["x"] == 0.0
    lost = g.clone()
    o = int(np.nonzero(~sub.any(1).numpy())[0][5])
    lost[o] = 0.0                                                    # a row of normal values
    _rejected(L.with_(go=go.numpy(), dx=_acc32(lost, slabs, L.nbr_t).to(td).float().numpy(), dw=dw(g)), "dx")


def test_recorder_catches_this_calls_dx_only():
    from findnpropagate_amd.spconv import conv as C

    class StandIn(torch.autograd.Function):      # the signature of SparseConvFunction, torch on the CPU, one offset
        @staticmethod
        def forward(ctx, feats, weight, rb, n_out_dev, n_in_dev, ranked=False, rows=None, prepacked=None):
            ctx.save_for_backward(feats, weight)
            return feats @ weight.reshape(weight.shape[0], -1).t()

        @staticmethod
        def backward(ctx, go):
            feats, weight = ctx.saved_tensors
            return go @ weight.reshape(weight.shape[0], -1), (go.t() @ feats).reshape(weight.shape), None, None, None, None, None, None

    rng = np.random.default_rng(2)
    x = torch.from_numpy(rng.standard_normal((50, 8)).astype(np.float32)).requires_grad_(True)
    w = torch.from_numpy(rng.standard_normal((8, 1, 1, 1, 8)).astype(np.float32)).requires_grad_(True)
    m = torch.from_numpy(rng.standard_normal((8, 8)).astype(np.float32))
    dy = torch.from_numpy(rng.standard_normal((50, 8)).astype(np.float32))
    n = torch.tensor([50], dtype=torch.int32)
    real = C.SparseConvFunction
    C.SparseConvFunction = StandIn
    try:
        with TT.Trace() as t:
            assert C.SparseConvFunction is t
            y = C.SparseConvFunction.apply(x, w, None, n, n, True, 50, None) + x @ m        # the input also feeds a residual branch
            t.backward((y * dy).sum())
        assert C.SparseConvFunction is StandIn
    finally:
        C.SparseConvFunction = real
    (rec,) = t.records
    own = dy @ w.detach().reshape(8, 8)
    assert torch.equal(rec._dx, own)                                  # this call's gradient ...
    assert torch.equal(x.grad, own + dy @ m.t()) and not torch.equal(x.grad, own)     # ... not the sum the tensor receives
    assert torch.equal(rec._go, dy) and torch.equal(rec._dw, w.grad) and torch.equal(rec._out, (x @ w.reshape(8, 8).t()).detach())
    assert rec.ranked and rec.rows == 50 and not rec.prepacked and torch.equal(rec._w, w.detach())
