"""The 16-bit TRAINING routes of the sparse convolution, layer by layer, against the float64 reference of tests/ref64.py (and
tests/ref32.py for an f32 layer).  A helper module, not a fixture; importing it needs no GPU.

RECORDER.  `Trace` is a context manager that needs no change of the product: it stands in for spconv.conv.SparseConvFunction (an
object with the same `apply` signature that calls the real function) and writes down, per call, the features as passed (after
cast and padding), the weight passed, the rulebook and the row counts, `ranked`, `rows`, whether `prepacked` was given, the
output, the output gradient AS IT ARRIVES (a hook on the output) and this call's own data gradient: a hook on an alias of the
input made for this call alone (`f.view_as(f)`), so that what is caught is this layer's gradient and not its sum with a residual
branch of the same tensor.  A forward hook on every SparseConvolution adds the module and the coordinates of both sides.  The
weight gradient is the module's `weight.grad` after the backward (each weight is used once per step, gradients cleared first).
While it is active the recorder also notes which of sparse.conv_forward / conv_dgrad / pack_weight_train / transposed_table the
function calls, with the route sparse.forward_route names for the very arguments of the call.

CHECKER.  `check_layer(record)` is a pure function of host arrays.  It builds the neighbour table from the COORDINATES
(ref64.neighbours_subm / neighbours_strided, match_rows for the strided output order), rounds the arrived gradient to the feature
dtype as the function does, and holds `out`, `dx` (stored in the feature dtype) and `dw` (f32, module layout) each to its own
derived bound, element by element, with no allowance.  A layer that was zero-padded (5 -> 16) is checked on the padded operands;
the module's gradient must equal the [..., :Cin] slice of that reference within the same bound.

SUBNORMALS.  ref64 assumes inputs without subnormals; a real fp16 gradient holds some, and nobody has measured how the matrix unit
treats them.  The reference is therefore evaluated on the values as they are, and an element's bound is widened by sum |x||w| over
its terms with a subnormal operand: the whole effect of flushing them to zero.  The share of such operands is reported per layer.

INTEGER INPUTS (`exact=True`): x, w and dy are small integers, every A is asserted below 2^24, and then `dw` must equal the
reference and `out` / `dx` the reference rounded once to the feature dtype, bit for bit."""
import hashlib
import time

import numpy as np
import torch

import ref32 as R32
import ref64 as R

HALF = (torch.bfloat16, torch.float16)
MIN_NORMAL = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14, torch.float32: 2.0 ** -126}


class Record:
    """one call of SparseConvFunction.apply.  `host()` fills the numpy fields the checker reads:
    x (rows, Cin) and w (Cout, kD, kH, kW, Cin) as passed, f32 (a 16-bit value is exact in f32); dtype: the features' torch dtype;
    out, go (the gradient as it arrived, f32 copy; go_dtype / go_contiguous: how it arrived), dx, dw (the MODULE's weight.grad) or
    None; n_in, n_out, cap_out, rows, ranked, prepacked; subm, ksize, stride, padding, batch, in_shape, out_shape, in_idx, out_idx."""

    def __init__(self, **kw):
        self.name = self.module = self.rb = None
        self.out = self.go = self.dx = self.dw = None
        self.go_dtype = self.go_contiguous = None
        self.ranked, self.rows, self.prepacked = False, None, False
        self.__dict__.update(kw)

    def adopt(self, other):
        """the module and the coordinates of `other`: for a call of the function that went past the module's forward"""
        for k in ("name", "module", "subm", "ksize", "stride", "padding", "batch", "in_shape", "out_shape", "_in_idx", "_out_idx"):
            setattr(self, k, getattr(other, k))
        return self

    def host(self):
        cpu = lambda t: None if t is None else t.detach().float().cpu().numpy()
        self.dtype = self._f.dtype
        self.x, self.w = cpu(self._f), cpu(self._w)
        self.out, self.dx = cpu(self._out), cpu(self._dx)
        if self._go is not None:
            self.go_dtype, self.go_contiguous = self._go.dtype, self._go.is_contiguous()
        self.go = cpu(self._go)
        g = self.module.weight.grad if self.module is not None else self._dw
        self.dw = cpu(g)
        self.n_in, self.n_out = int(self._n_in_dev.item()), int(self._n_out_dev.item())
        self.cap_out = int(self.rb.cap_out)
        self.in_idx = self._in_idx.cpu().numpy()
        self.out_idx = self.in_idx if self.subm else self._out_idx.cpu().numpy()
        return self


class Trace:
    """with Trace(net) as t: forward; t.backward(loss) -> t.records (in call order), t.calls (what the function called)"""

    SPIED = ("conv_forward", "conv_dgrad", "pack_weight_train", "transposed_table")

    def __init__(self, net=None):
        self.net, self.records, self.calls, self.phase = net, [], [], "forward"
        self._handles, self._open = [], {}

    # ---- the stand-in for SparseConvFunction
    def apply(self, f, weight, rb, n_out_dev, n_in_dev, ranked=False, rows=None, prepacked=None):
        rec = Record(rb=rb, ranked=bool(ranked), rows=rows, prepacked=prepacked is not None, _f=f.detach(), _w=weight.detach().clone(),
                     _n_out_dev=n_out_dev, _n_in_dev=n_in_dev, _go=None, _dx=None, _dw=None, _out=None)
        self.records.append(rec)
        fa = f
        if f.requires_grad:
            fa = f.view_as(f)         # an alias for this call alone: its gradient is this layer's dx and nothing else
            fa.register_hook(lambda g: setattr(rec, "_dx", g.detach()))
        if weight.requires_grad and weight.is_leaf:
            self._handles.append(weight.register_hook(lambda g: setattr(rec, "_dw", g.detach().clone())))
        out = self._real.apply(fa, weight, rb, n_out_dev, n_in_dev, ranked, rows, prepacked)
        rec._out = out.detach()
        if out.requires_grad:
            out.register_hook(lambda g: setattr(rec, "_go", g.detach()))
        return out

    # ---- context
    def __enter__(self):
        from findnpropagate_amd import sparse as S
        from findnpropagate_amd.spconv import conv as C
        self._C, self._S, self._real = C, S, C.SparseConvFunction
        C.SparseConvFunction = self
        if self.net is not None:
            for name, m in self.net.named_modules():
                if isinstance(m, C.SparseConvolution):
                    self._handles.append(m.register_forward_pre_hook(self._pre))
                    self._handles.append(m.register_forward_hook(lambda m, inp, out, name=name: self._post(name, m, inp[0], out)))
        self._spied = {n: getattr(S, n) for n in self.SPIED}
        for n in self.SPIED:
            setattr(S, n, getattr(self, "_spy_" + n))
        return self

    def __exit__(self, *exc):
        self._C.SparseConvFunction = self._real
        for n, fn in self._spied.items():
            setattr(self._S, n, fn)
        for h in self._handles:
            h.remove()
        return False

    def _pre(self, m, inp):
        self._open[id(m)] = len(self.records)

    def _post(self, name, m, x, out):
        first = self._open.pop(id(m))
        assert len(self.records) == first + 1, f"{name}: {len(self.records) - first} calls of the function in one forward"
        rec = self.records[first]
        rec.name, rec.module, rec.subm = name or type(m).__name__, m, bool(m.subm)
        rec.ksize, rec.stride, rec.padding = list(m.kernel_size), list(m.stride), list(m.padding)
        rec.batch, rec.in_shape, rec.out_shape = x.batch_size, list(x.spatial_shape), list(out.spatial_shape)
        rec._in_idx, rec._out_idx = x.indices, out.indices

    def backward(self, tensor, gradient=None):
        self.phase = "backward"
        try:
            tensor.backward(gradient)
        finally:
            self.phase = "forward"

    def host(self):
        return [r.host() for r in self.records]

    def called(self, fn, phase=None):
        return [c for c in self.calls if c["fn"] == fn and (phase is None or c["phase"] == phase)]

    # ---- what the function calls of sparse.py, with the route named for the call's own arguments
    def _spy_conv_forward(self, feat_in, w_packed, rb, n_out_dev, out_dtype=None, scale=None, shift=None, residual=None, relu=False, out=None,
                          ranked=False, valu=False, tile=None):
        K, Cout, Cin = w_packed.shape
        od = out.dtype if out is not None else (out_dtype or feat_in.dtype)
        route = self._S.forward_route(rb, K, Cin, Cout, feat_in.dtype, od, feat_in.shape[0], ranked, tile, valu)
        self.calls.append(dict(fn="conv_forward", phase=self.phase, route=route, rb=rb, w=w_packed, ranked=bool(ranked), rows=feat_in.shape[0]))
        return self._spied["conv_forward"](feat_in, w_packed, rb, n_out_dev, out_dtype=out_dtype, scale=scale, shift=shift, residual=residual,
                                           relu=relu, out=out, ranked=ranked, valu=valu, tile=tile)

    def _spy_conv_dgrad(self, grad_out, w_packed, nbr_t, n_in_dev, cap_in, pretransposed=False):
        self.calls.append(dict(fn="conv_dgrad", phase=self.phase, table=nbr_t, w=w_packed, pretransposed=bool(pretransposed), cap_in=cap_in))
        return self._spied["conv_dgrad"](grad_out, w_packed, nbr_t, n_in_dev, cap_in, pretransposed=pretransposed)

    def _spy_pack_weight_train(self, weight, dtype, mirror=0):
        self.calls.append(dict(fn="pack_weight_train", phase=self.phase, dtype=dtype, mirror=mirror))
        return self._spied["pack_weight_train"](weight, dtype, mirror)

    def _spy_transposed_table(self, rb, n_out_dev, cap_in):
        had = rb._nbr_t
        t = self._spied["transposed_table"](rb, n_out_dev, cap_in)
        self.calls.append(dict(fn="transposed_table", phase=self.phase, rb=rb, cap_in=cap_in, remade=t is not had))
        return t


# ------------------------------------------------------------------------------------------------ the checker
class Result:
    def __init__(self, name):
        self.name, self.ratio, self.fails, self.sub, self.min_share, self.t_ref = name, {}, [], {}, None, 0.0

    def line(self):
        f = lambda q: "-" if q not in self.ratio else f"{self.ratio[q]:.4g}"
        return f"out {f('out')} / dx {f('dx')} / dw {f('dw')}"


def _sub(a, td):
    """mask of the subnormal entries of `a` in the type td"""
    m = np.abs(a)
    return (m > 0) & (m < MIN_NORMAL[td])


def _abs_conv(xa, wa, nbr):
    """sum |x||w| of ref64.conv for non-negative f64 tensors xa (n_in, Cin), wa (K, Cout, Cin)"""
    A = torch.zeros((nbr.shape[1], wa.shape[1]), dtype=torch.float64)
    for k in range(nbr.shape[0]):
        o = np.nonzero(nbr[k] >= 0)[0]
        if o.shape[0]:
            A.index_add_(0, torch.from_numpy(o), xa[torch.from_numpy(np.ascontiguousarray(nbr[k][o]))] @ wa[k].T)
    return A


def _abs_wgrad(xa, ga, nbr):
    A = torch.zeros((nbr.shape[0], ga.shape[1], xa.shape[1]), dtype=torch.float64)
    for k in range(nbr.shape[0]):
        o = np.nonzero(nbr[k] >= 0)[0]
        if o.shape[0]:
            A[k] = ga[torch.from_numpy(o)].T @ xa[torch.from_numpy(np.ascontiguousarray(nbr[k][o]))]
    return A


def _split(a, td):
    """(|a| on its normal entries, |a| on its subnormal entries) as f64 tensors, or (None, None) without subnormals"""
    s = _sub(a, td)
    if not s.any():
        return None, None
    m = torch.from_numpy(np.abs(a).astype(np.float64))
    st = torch.from_numpy(s)
    return m * ~st, m * st


def _widen_conv(x, w, nbr, td):
    """sum |x||w| over the terms of a convolution with a subnormal operand (0 when there is none)"""
    xn, xs = _split(x, td)
    wn, ws = _split(w, td)
    if xs is None and ws is None:
        return 0.0
    xa = torch.from_numpy(np.abs(x).astype(np.float64))
    wa = torch.from_numpy(np.abs(w).astype(np.float64))
    A = 0.0
    if xs is not None:
        A = A + _abs_conv(xs, wa, nbr)                       # a subnormal x with any w
    if ws is not None:
        A = A + _abs_conv(xa if xn is None else xn, ws, nbr)    # a normal x with a subnormal w
    return A


def _widen_wgrad(x, g, nbr, td_x, td_g):
    xn, xs = _split(x, td_x)
    gn, gs = _split(g, td_g)
    if xs is None and gs is None:
        return 0.0
    xa = torch.from_numpy(np.abs(x).astype(np.float64))
    ga = torch.from_numpy(np.abs(g).astype(np.float64))
    A = 0.0
    if gs is not None:
        A = A + _abs_wgrad(xa, gs, nbr)
    if xs is not None:
        A = A + _abs_wgrad(xs, ga if gn is None else gn, nbr)
    return A


def reference_table(rec):
    """the neighbour table (K, n_out) of a record from its COORDINATES, in the device's output row order"""
    idx = rec.in_idx[:rec.n_in]
    if rec.subm:
        assert rec.n_out == rec.n_in
        return R.neighbours_subm(idx, rec.batch, rec.in_shape, rec.ksize)
    out, osh, nbr = R.neighbours_strided(idx, rec.batch, rec.in_shape, rec.ksize, rec.stride, rec.padding)
    assert list(osh) == list(rec.out_shape), (osh, rec.out_shape)
    assert out.shape[0] == rec.n_out, ("output sites", out.shape[0], rec.n_out)
    order = R.match_rows(out, rec.out_idx[:rec.n_out], osh)
    return np.ascontiguousarray(nbr[:, order])


def _round_to(a, td):
    """f32 array rounded to td (nearest even), nothing flushed; f32"""
    return a if td == torch.float32 else torch.from_numpy(np.ascontiguousarray(a)).to(td).float().numpy()


def check_layer(rec, exact=False, memo=None):
    """-> Result: the worst err / bound of out, dx and dw (those the record holds), every failure as '<layer>: <quantity>: ...',
    the shares of subnormal operands and the smallest share of rows any offset has a pair for.
    memo: a dict that keeps the reference sums between records with the same operands and table (keyed by their bytes)."""
    res = Result(rec.name)
    td = rec.dtype
    half = td in HALF
    assert half or not exact
    t0 = time.perf_counter()
    nbr = reference_table(rec)
    K, n_in, n_out = nbr.shape[0], rec.n_in, rec.n_out
    res.min_share = float((nbr >= 0).mean(1).min()) if n_out else 0.0
    Cout, Cin = rec.w.shape[0], rec.w.shape[-1]
    x = np.ascontiguousarray(rec.x[:n_in])
    wq = _round_to(rec.w, td)
    wp = np.ascontiguousarray(wq.reshape(Cout, K, Cin).transpose(1, 0, 2))
    g = None if rec.go is None else np.ascontiguousarray(_round_to(rec.go, td)[:n_out])
    res.sub = {"x": float(_sub(x, td).mean()), "w": float(_sub(wp, td).mean()), "go": 0.0 if g is None else float(_sub(g, td).mean())}
    key = None
    if memo is not None:
        h = hashlib.sha1()
        for a in (nbr, x, wp) + (() if g is None else (g,)):
            h.update(np.ascontiguousarray(a).tobytes())
        key = (h.hexdigest(), str(td), rec.dx is not None, rec.dw is not None)
    sums = memo.get(key) if key is not None else None
    if sums is None:
        sums = {"out": R.conv(x, wp, nbr)}
        if g is not None and rec.dx is not None:
            sums["dx"] = R.dgrad(g, wp, nbr, n_in)
        if g is not None and rec.dw is not None:
            sums["dw"] = R.wgrad(x, g, nbr)
        if key is not None:
            memo[key] = sums
    epi = (lambda s, od, P=0: R.epilogue(s, out_dtype=od)) if half else (lambda s, od, P=0: R32.epilogue(s, out_dtype=od, P=P))
    u_out = R.U16[td] if half else 0.0

    def hold(q, got, s, od, n, widen, P=0):
        if exact:
            assert float(s.A.max()) < 2 ** 24, (rec.name, q, float(s.A.max()))
            V = s.S if od == torch.float32 else R32.exact16(s.S, od).double()
            e = torch.zeros_like(s.S)
        else:
            V, e = epi(s, od, P)
            e = e + (1.0 + (u_out if od != torch.float32 else 0.0)) * widen
        worst, rep = R.check(got, V, e, n)
        res.ratio[q] = worst
        if rep is not None:
            res.fails.append(f"{rec.name}: {q}: {rep}")

    hold("out", rec.out, sums["out"], td, n_out, 0.0 if exact else _widen_conv(x, wp, nbr, td))
    if "dx" in sums:
        nbr_t = R.transpose_nbr(nbr, n_in)
        wt = np.ascontiguousarray(wp.transpose(0, 2, 1))
        hold("dx", rec.dx, sums["dx"], td, n_in, 0.0 if exact else _widen_conv(g, wt, nbr_t, td))
    elif rec.dx is not None:
        res.fails.append(f"{rec.name}: dx: a data gradient without an output gradient")
    if "dw" in sums:
        # what conv_wgrad adds up: the chunk partials of the f32 kernels (ref32.wgrad_partials; the few-pairs kernel on pair lists)
        P = 0 if half else R32.wgrad_partials(min(rec.cap_out, rec.go.shape[0]), Cin, Cout, K, Cin * Cout <= 128)
        cm = rec.dw.shape[-1]          # the module's own input channels: fewer than Cin where the layer was zero-padded
        if rec.dw.shape != (Cout, *rec.w.shape[1:4], cm) or cm > Cin:
            res.fails.append(f"{rec.name}: dw: weight.grad has shape {rec.dw.shape}, the module's weight {(Cout, *rec.w.shape[1:4], cm)}")
        else:
            s = sums["dw"]
            s = R.Sums(s.S[..., :cm], s.A[..., :cm], s.T)
            widen = 0.0 if exact else _widen_wgrad(x, g, nbr, td, td)
            if not isinstance(widen, float):
                widen = widen[..., :cm]
            hold("dw", torch.from_numpy(rec.dw.reshape(Cout, K, cm)).permute(1, 0, 2), s, torch.float32, None, widen, P)
    res.t_ref = time.perf_counter() - t0
    return res


def check_step(case, records, exact=False, memo=None):
    """check_layer on every record; prints `RATIO <case> | <layer> | out / dx / dw` and the subnormal shares per layer and
    returns (results, all failures of the step)"""
    results, fails = [], []
    for rec in records:
        r = check_layer(rec, exact=exact, memo=memo)
        print(f"RATIO {case} | {r.name} | {r.line()}")
        if any(r.sub.values()):
            print(f"SUBNORMAL {case} | {r.name} | x {r.sub['x']:.3g} / w {r.sub['w']:.3g} / grad_out {r.sub['go']:.3g} of the operands")
        results.append(r)
        fails += r.fails
    return results, fails
