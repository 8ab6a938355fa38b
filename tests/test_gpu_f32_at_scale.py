"""The f32 engine's kernels (csrc/spconv_f32.hip; spconv_first_kernel and spconv_valu_kernel of csrc/spconv.hip; the f32 and mixed
weight gradients of csrc/spconv_bwd.hip) against the float64 reference of tests/ref64.py under the f32 bound of tests/ref32.py,
AT THE SIZES AT WHICH THEIR LAUNCH CODE CHANGES FORM: full tiles of the persistent loop, the evenly cut short ranges (bpw blocks
per wave), thin inputs under a large grid, q = 2 rows per thread of the class sort, the second grid-stride round of the first
layer, 24 / 32 / 128 chunks of a weight gradient with empty trailing chunks.  Every other value check of these kernels against
anything independent stops at 6 000 rows.

Per case: every caller-owned output is prefilled with NaN; the rows of x, residual and dy behind n are NaN; there is spare
capacity behind n and n is no multiple of 16; the regime the case is written for is ASSERTED from the restated geometry
(ref32) and printed.  There is no allowance: every element of every row below n is checked —
  * random f32 data against the derived bound (ref32's docstring), all four epilogue forms;
  * the oracle's fmaf chain on the chosen rows (ref32.chain_rows), array_equal, plain and res-bn-relu;
  * integer inputs bit for bit on all rows (bound zero);
  * equal bits between the plain and the 4 x 4-transposed weight layout, the sorted and the plain sweep, the VALU and the matrix
    chain, and two runs of a weight gradient.
The err / bound ratios each case prints are for the record, never a criterion."""
import time

import numpy as np
import pytest
import torch

import ref32 as R32
import ref64 as R
from findnpropagate_amd import sparse as S
from test_gpu_conv_at_scale import FORMS, Recorder, _strided_setup, sites

pytestmark = pytest.mark.gpu

F32 = torch.float32
PLAIN, BN_RELU, RES_BN_RELU, RES = FORMS


def _dev(a, cuda, td=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return t if td is None else t.to(td)


def _dev_nan(a, cap, cuda, td=None):
    """(cap, C) on the device: the rows of `a`, NaN behind them"""
    t = torch.full((cap, a.shape[1]), float("nan"), dtype=td or F32, device=cuda)
    t[:a.shape[0]] = _dev(a, cuda, td)
    return t


def _n_full(cout):
    """rows for two full tiles per workgroup plus a partial one, not a multiple of 16"""
    ft = R32.full_tile_cap(cout)
    n = 2 * ft + int(0.3 * ft) // 16 * 16 + 5
    assert n % 16 == 5 and n > 2 * ft
    return n


def _regime(rec, n, cap, cout):
    """the grid and what its ranges are: (G, blocks of the shortest and longest non-empty range, passes of the persistent loop)"""
    G = R32.grid_of(cap, cout)
    rb, re = R32.ranges(n, G)
    blk = (re - rb + 15) >> 4
    live = blk[blk > 0]
    info = dict(G=G, live=int(live.shape[0]), lo=int(live.min()), hi=int(live.max()), small=bool((live < 4 * R32.mb(cout)).all()),
                full=bool((live >= 4 * R32.mb(cout)).all()), passes=int(-(-int(live.max()) * 16 // R32.tile_rows(cout))))
    print(f"REGIME {rec.case} | grid {G} of {R32.resident(cout)} resident | {info['live']} live ranges of {info['lo']} .. {info['hi']} blocks | "
          f"{'small' if info['small'] else 'full tiles' if info['full'] else 'both forms'} | {info['passes']} pass(es)")
    return info


class Case:
    """the random and the integer inputs of one layer on the device (NaN behind the rows), their reference sums, and the checks"""

    def __init__(self, rec, cuda, oracle, cin, cout, ksize, rows_in, cap_in, n, cap, nbr, tile, res16=False):
        rng = np.random.default_rng(99)
        self.rec, self.cuda, self.oracle, self.cin, self.cout, self.n, self.cap, self.nbr, self.tile = rec, cuda, oracle, cin, cout, n, cap, nbr, tile
        self.rows_in, self.sets = rows_in, {}
        for name, draw in (("random", R32.draw32), ("integer", R32.draw32_exact)):
            d = draw(rng, rows_in, n, cin, cout, ksize)
            if res16 and name == "random":       # (a 16-bit output adds a residual of its own type: values both types hold)
                d["res"] = R.round16(R.round16(d["res"], torch.bfloat16), torch.float16)
            t0 = time.perf_counter()
            sums = R.conv(d["x"], d["wp"], nbr)
            rec.t_ref += time.perf_counter() - t0
            if name == "integer":
                R32.assert_exactly_summable(sums)
            w = _dev(d["w"], cuda)
            dev = dict(x=_dev_nan(d["x"], cap_in, cuda), wp=S.pack_weight(w, F32), wperm=S.pack_weight(w, F32, mfma_f32=True), sc=_dev(d["sc"], cuda),
                       sh=_dev(d["sh"], cuda), res=_dev_nan(d["res"], cap, cuda))
            assert np.array_equal(dev["wp"].cpu().numpy(), d["wp"])
            self.sets[name] = (d, sums, dev)

    def call(self, fn, name, form, od=F32):
        _, res, scaled, relu = form
        dev = self.sets[name][2]
        out = torch.full((self.cap, self.cout), float("nan"), dtype=od, device=self.cuda)
        residual = None if not res else dev["res"] if od == F32 else dev["res"].to(od)
        got = fn(dev, dev["sc"] if scaled else None, dev["sh"] if scaled else None, residual, relu, out)
        assert got.dtype == od and got.data_ptr() == out.data_ptr()
        return got

    def ref(self, name, form, od=F32):
        _, res, scaled, relu = form
        d, sums, _ = self.sets[name]
        t0 = time.perf_counter()
        V, e = R32.epilogue(sums, d["sc"] if scaled else None, d["sh"] if scaled else None, d["res"] if res else None, relu, od)
        if name == "integer":
            V, e = (V if od == F32 else R32.exact16(V, od).double()), torch.zeros_like(V)
        self.rec.t_ref += time.perf_counter() - t0
        return V, e

    def chain(self, path, got, form, rows):
        _, res, scaled, relu = form
        d = self.sets["random"][0]
        t0 = time.perf_counter()
        want = R32.oracle_rows(self.oracle, d["x"], d["w"], self.nbr, rows, d["sc"] if scaled else None, d["sh"] if scaled else None,
                               d["res"] if res else None, relu)
        self.rec.t_ref += time.perf_counter() - t0
        have = got[torch.from_numpy(rows).to(got.device)].cpu().numpy()
        bad = rows[(have != want).any(1) | np.isnan(have).any(1)]
        print(f"CHAIN {self.rec.case} | {path} {form[0]} | {rows.shape[0]} rows, {bad.shape[0]} differ")
        if bad.shape[0]:
            self.rec.fail.append(f"{path} {form[0]}: {bad.shape[0]} of {rows.shape[0]} chosen rows are not the oracle's bits, first {bad[:12].tolist()}")

    def run(self, path, fn, forms=FORMS, chain=None, od=F32, exact_forms=None):
        """fn(dev, scale, shift, residual, relu, out) -> out.  Random data: the bound in every form, the chain on the rows `chain`
        in the plain and res-bn-relu forms; integer data: bit for bit, in those two forms (or `exact_forms`).  Returns the outputs by (data, form name)."""
        outs = {}
        chain_forms = (forms[0], RES_BN_RELU if RES_BN_RELU in forms else forms[-1])      # (a strided layer has no residual: bn-relu)
        for form in forms:
            got = outs["random", form[0]] = self.call(fn, "random", form, od)
            self.rec.check(f"{path} {form[0]}", got, *self.ref("random", form, od), self.n, self.tile)
            if chain is not None and form in chain_forms and od == F32:
                self.chain(path, got, form, chain)
        for form in (dict.fromkeys(chain_forms) if exact_forms is None else exact_forms):
            got = outs["integer", form[0]] = self.call(fn, "integer", form, od)
            self.rec.check(f"{path} integers {form[0]}", got, *self.ref("integer", form, od), self.n, self.tile)
        return outs

    def same(self, what, a, b):
        if not torch.equal(a[:self.n], b[:self.n]):
            rows = torch.nonzero((a[:self.n] != b[:self.n]).any(1)).reshape(-1)
            self.rec.fail.append(f"{what}: {rows.numel()} rows differ in their bits, first {rows[:12].tolist()}")
        print(f"EQUAL {self.rec.case} | {what}")


def _subm(cuda, kind, n, cap, order, masks=False):
    idx, B, shape = sites(kind, n, order)
    d_idx = _dev(np.concatenate([idx, np.zeros((cap - n, 4), np.int32)]), cuda)
    n_dev = S.device_scalar(n, cuda)
    grid = S.build_grid(d_idx, n_dev, B, shape)
    rb = S.rulebook_subm(d_idx, n_dev, grid, 3, masks=masks)
    assert rb.cap_out == cap and getattr(rb, "_perm_f32", None) is None and not getattr(rb, "_lean", False)
    return idx, B, shape, d_idx, n_dev, grid, rb


def _forward(rb, n_dev, weight="wp", **kw):
    return lambda dev, sc, sh, r, relu, out: S.conv_forward(dev["x"], dev[weight], rb, n_dev, scale=sc, shift=sh, residual=r, relu=relu, out=out, **kw)


def _mfma_case(rec, cuda, oracle, cin, cout, ksize, rows_in, cap_in, n, cap, nbr, rb, n_dev, forms, G):
    """the checks of a forward case on the matrix kernel: bound, chain, integers, and the transposed weight layout"""
    assert (cin, cout) in S.F32_MFMA_SHAPES
    c = Case(rec, cuda, oracle, cin, cout, ksize, rows_in, cap_in, n, cap, nbr, R32.tile_rows(cout))
    rows = R32.chain_rows(n, cout, G, np.random.default_rng(3))
    outs = c.run("mfma", _forward(rb, n_dev), forms, chain=rows)
    assert isinstance(c.sets["random"][2]["wperm"], S.PermutedWeight)
    form = RES_BN_RELU if RES_BN_RELU in forms else forms[-1]
    for name in ("random", "integer"):
        c.same(f"transposed weight layout, {name} {form[0]}", c.call(_forward(rb, n_dev, "wperm"), name, form), outs[name, form[0]])
    return c, outs, rows


# ------------------------------------------------------------------------------------------------ forward, full tiles
@pytest.mark.parametrize("C,kind,order", [(16, "sheet", "rank"), (32, "mixed", "random"), (64, "solid", "rank"), (128, "sheet", "rank")])
def test_forward_full_tiles_subm(cuda, oracle, C, kind, order):
    """the persistent loop of spconv_mfma_f32_kernel: every workgroup runs two full tiles and a partial one"""
    n, spare = _n_full(C), 3000
    cap = n + spare
    rec = Recorder(f"f32 subm {C}->{C} {kind}/{order} n={n} cap={cap}")
    reg = _regime(rec, n, cap, C)
    assert cap >= R32.full_tile_cap(C) and reg["G"] == R32.resident(C) and reg["full"] and reg["passes"] == 3 and reg["lo"] > 2 * 4 * R32.mb(C)
    idx, B, shape, d_idx, n_dev, grid, rb = _subm(cuda, kind, n, cap, order)
    _mfma_case(rec, cuda, oracle, C, C, 3, n, cap, n, cap, R.neighbours_subm(idx, B, shape), rb, n_dev, FORMS, reg["G"])
    rec.done()


STRIDED = {   # (B, shape, density, k, s, p): output sites above two full tiles per workgroup and a partial one, not a multiple of 16
    (16, 32): (3, [13, 400, 398], 0.1, 3, 2, 1),
    (32, 64): (2, [13, 330, 330], 0.1, 3, 2, 1),
    (64, 128): (2, [13, 280, 280], 0.1, 3, 2, 1),
    (128, 128): (2, [5, 260, 260], 0.6, (3, 1, 1), (2, 1, 1), 0),      # conv_out: the run-time-K instance
}


@pytest.mark.parametrize("cin,cout", list(STRIDED))
def test_forward_full_tiles_strided(cuda, oracle, cin, cout):
    """the channel-doubling layers and conv_out on strided tables (rows of the input in random order: the grid carries a
    permutation); a strided layer has no residual"""
    B, shape, density, k, s, p = STRIDED[cin, cout]
    spare = 2000
    idx, n_in, m, d_idx, n_dev, grid, rb, nbr = _strided_setup(cuda, B, shape, density, k, s, p, spare)
    cap = m + spare
    rec = Recorder(f"f32 strided {cin}->{cout} k={k} n_in={n_in} n_out={m} cap={cap}")
    reg = _regime(rec, m, cap, cout)
    assert m % 16 and m >= _n_full(cout) and reg["G"] == R32.resident(cout) and reg["full"] and reg["passes"] >= 3
    _mfma_case(rec, cuda, oracle, cin, cout, k, n_in, n_in, m, cap, nbr, rb, rb.out_n, [PLAIN, BN_RELU], reg["G"])
    rec.done()


# ------------------------------------------------------------------------------------------------ forward, short ranges
@pytest.mark.parametrize("C", [16, 64, 128])
@pytest.mark.parametrize("blocks", ["4 MB - 1", "5"])
def test_forward_short_ranges_cut_over_the_waves(cuda, oracle, C, blocks):
    """tiles < resident <= fine: the persistent grid with ranges shorter than a tile, cut evenly over the four waves — ranges of
    4 MB - 1 blocks (bpw = MB, the last wave one block short) and of 5 blocks (bpw = 2: 2, 2, 1 and a wave with nothing)"""
    G, MB = R32.resident(C), R32.mb(C)
    L = 4 * MB - 1 if blocks == "4 MB - 1" else 5
    n, spare = L * G * 16 - 11, 3000
    cap = n + spare
    rec = Recorder(f"f32 subm {C}->{C} ranges of {L} blocks n={n} cap={cap}")
    reg = _regime(rec, n, cap, C)
    assert -(-cap // R32.tile_rows(C)) < G <= -(-cap // 64) and reg["G"] == G and reg["small"] and reg["lo"] == reg["hi"] == L and reg["live"] == G
    rb0, re0 = R32.ranges(n, G)
    small, bpw, plan = R32.wave_plan(int(rb0[7]), int(re0[7]), C)
    assert small and bpw == (MB if L != 5 else 2) and [sum(b - a for a, b in w) // 16 for w in plan] == ([MB, MB, MB, MB - 1] if L != 5 else [2, 2, 1, 0])
    idx, B, shape, d_idx, n_dev, grid, rb = _subm(cuda, "sheet", n, cap, "rank")
    _mfma_case(rec, cuda, oracle, C, C, 3, n, cap, n, cap, R.neighbours_subm(idx, B, shape), rb, n_dev, FORMS, G)
    rec.done()


@pytest.mark.parametrize("C", [16, 128])
def test_forward_thin_input_under_a_large_grid(cuda, oracle, C):
    """n in {1, 17, 400} under a capacity of the full-tile regime: the persistent grid, most of its ranges empty"""
    cap = R32.full_tile_cap(C) + 3000
    rec = Recorder(f"f32 subm {C}->{C} thin input cap={cap}")
    for n in (1, 17, 400):
        reg = _regime(rec, n, cap, C)
        assert reg["G"] == R32.resident(C) and reg["live"] == -(-n // 16) < reg["G"] and reg["hi"] == 1
        idx, B, shape, d_idx, n_dev, grid, rb = _subm(cuda, "sheet", n, cap, "rank")
        c = Case(rec, cuda, oracle, C, C, 3, n, cap, n, cap, R.neighbours_subm(idx, B, shape), R32.tile_rows(C))
        outs = c.run(f"n={n} mfma", _forward(rb, n_dev), [PLAIN, BN_RELU, RES_BN_RELU], chain=np.arange(n))
        c.same(f"n={n} transposed weight layout", c.call(_forward(rb, n_dev, "wperm"), "random", RES_BN_RELU), outs["random", RES_BN_RELU[0]])
    rec.done()


# ------------------------------------------------------------------------------------------------ class-sorted sweep
SORTED = [(16, S.F32_SORT_MIN_ROWS + 3005, 1), (32, S.F32_SORT_MIN_ROWS + 3005, 1),
          (16, 1024 * 1024 + 104861, 2), (64, 1024 * 512 + 52437, 2)]


@pytest.mark.parametrize("C,n,q", SORTED)
def test_class_sorted_sweep(cuda, oracle, C, n, q):
    """fnp_rulebook_classsort_f32 + fnp_spconv_forward_f32_sorted: perm against the restated ranges on the CPU (classes from the
    COORDINATES), the sorted output against the reference, the chain and the plain sweep; q = 2 rows per thread of the sort"""
    spare = 3000
    cap = n + spare
    assert n % 16 and cap >= S.F32_SORT_MIN_ROWS and S.f32_sorted_by_default(C, F32, cap)
    rec = Recorder(f"f32 sorted {C}->{C} n={n} cap={cap}")
    reg = _regime(rec, n, cap, C)
    G = reg["G"]
    qs = R32.sort_q(n, G)
    assert int(qs.max()) == q and reg["hi"] * 16 <= R32.SORT_THREADS * R32.SORT_Q_MAX and (q == 1 or int(qs.min()) == 2)
    print(f"REGIME {rec.case} | class sort: {q} row(s) per thread")
    idx, B, shape, d_idx, n_dev, grid, rb0 = _subm(cuda, "sheet", n, cap, "rank")
    rb = S.rulebook_subm(d_idx, n_dev, grid, 3, masks=True)
    assert torch.equal(rb.nbr[:, :n], rb0.nbr[:, :n])
    S.classsort_f32(rb, n_dev, C)
    assert rb._perm_f32 is not None and rb._perm_f32.get(C) is not None, "the sorted sweep did not get its order: conv_forward would run the plain kernel"
    nbr = R.neighbours_subm(idx, B, shape)
    cls = R32.zclass(nbr)
    assert np.unique(cls).shape[0] >= 3
    R32.check_perm(rb._perm_f32[C][:n].cpu().numpy(), cls, n, G)
    c = Case(rec, cuda, oracle, C, C, 3, n, cap, n, cap, nbr, R32.tile_rows(C))
    rows = R32.chain_rows(n, C, G, np.random.default_rng(3))
    outs = c.run("sorted", _forward(rb, n_dev, ranked=True), FORMS, chain=rows, exact_forms=FORMS)
    for name in ("random", "integer"):
        for form in FORMS:
            c.same(f"sorted against plain sweep, {name} {form[0]}", outs[name, form[0]], c.call(_forward(rb0, n_dev, ranked=True), name, form))
    c.same("sorted, transposed weight layout", c.call(_forward(rb, n_dev, "wperm", ranked=True), "random", RES_BN_RELU), outs["random", RES_BN_RELU[0]])
    rec.done()


# ------------------------------------------------------------------------------------------------ conv_input
def test_conv_input_first_kernel(cuda, oracle):
    """spconv_first_kernel (5 -> 16): two grid-stride rounds of 2048 x 256 rows and a partial third, f32 / bf16 / fp16 outputs (one
    reference for the three)"""
    n = 2 * R32.FIRST_ROUND_ROWS + int(0.3 * R32.FIRST_ROUND_ROWS) // 16 * 16 + 5
    spare = 3000
    cap = n + spare
    assert n > 1048576 + 5 and n % 16 and -(-cap // 256) > 2048
    rec = Recorder(f"f32 conv_input 5->16 n={n} cap={cap}")
    print(f"REGIME {rec.case} | grid 2048 workgroups of 256 rows | {-(-n // R32.FIRST_ROUND_ROWS)} grid-stride rounds")
    idx, B, shape, d_idx, n_dev, grid, rb = _subm(cuda, "sheet", n, cap, "rank")
    nbr = R.neighbours_subm(idx, B, shape)
    rows = R32.rows_around(n, [R32.FIRST_ROUND_ROWS, 2 * R32.FIRST_ROUND_ROWS], np.random.default_rng(3))
    c = Case(rec, cuda, oracle, 5, 16, 3, n, cap, n, cap, nbr, 256, res16=True)
    for od in (F32, torch.bfloat16, torch.float16):
        fwd = lambda dev, sc, sh, r, relu, out: S.conv_forward(dev["x"], dev["wp"], rb, n_dev, out_dtype=out.dtype, scale=sc, shift=sh, residual=r,
                                                               relu=relu, out=out)
        c.run(f"first {str(od)[6:]} out", fwd, FORMS if od == F32 else [BN_RELU, RES_BN_RELU], chain=rows, od=od)
    rec.done()


# ------------------------------------------------------------------------------------------------ the thread-per-element chain
def test_valu_chain_on_a_matrix_shape(cuda, oracle):
    """valu=True on 16 -> 16 at its full-tile size: the chain, and the matrix kernel's bits"""
    C = 16
    n, spare = _n_full(C), 3000
    cap = n + spare
    rec = Recorder(f"f32 valu {C}->{C} n={n} cap={cap}")
    per = R32.valu_round_elements(cap, C)
    print(f"REGIME {rec.case} | {-(-n * C // per)} grid-stride rounds of {per} elements")
    assert n * C > 2 * per
    idx, B, shape, d_idx, n_dev, grid, rb = _subm(cuda, "lattice", n, cap, "rank")
    nbr = R.neighbours_subm(idx, B, shape)
    c = Case(rec, cuda, oracle, C, C, 3, n, cap, n, cap, nbr, R32.tile_rows(C))
    rows = np.union1d(R32.chain_rows(n, C, R32.grid_of(cap, C), np.random.default_rng(3)),
                      R32.rows_around(n, [j * per // C for j in range(1, n * C // per + 1)], np.random.default_rng(4)))
    outs = c.run("valu", _forward(rb, n_dev, valu=True), [PLAIN, RES_BN_RELU], chain=rows)
    for name in ("random", "integer"):
        for form in (PLAIN, RES_BN_RELU):
            c.same(f"valu against mfma, {name} {form[0]}", outs[name, form[0]], c.call(_forward(rb, n_dev), name, form))
    rec.done()


def test_valu_chain_on_a_shape_without_a_matrix_kernel(cuda, oracle):
    """24 -> 40 at 150 000 rows: what runs behind the 32-bit offset limit and for every shape the matrix kernel does not cover"""
    cin, cout, n, spare = 24, 40, 150005, 3000
    cap = n + spare
    assert (cin, cout) not in S.F32_MFMA_SHAPES
    rec = Recorder(f"f32 valu {cin}->{cout} n={n} cap={cap}")
    per = R32.valu_round_elements(cap, cout)
    print(f"REGIME {rec.case} | {-(-n * cout // per)} grid-stride rounds of {per} elements")
    assert n * cout > 2 * per
    idx, B, shape, d_idx, n_dev, grid, rb = _subm(cuda, "sheet", n, cap, "rank")
    nbr = R.neighbours_subm(idx, B, shape)
    c = Case(rec, cuda, oracle, cin, cout, 3, n, cap, n, cap, nbr, 256)
    rows = R32.rows_around(n, [j * per // cout for j in range(1, n * cout // per + 1)], np.random.default_rng(3), random_rows=2000)
    c.run("valu", _forward(rb, n_dev), FORMS, chain=rows)
    rec.done()


# ------------------------------------------------------------------------------------------------ data gradient
def _dgrad_case(rec, cuda, cin, cout, ksize, n_in, cap_in, m, cap_out, nbr, run):
    """run(dy (cap_out, Cout) on the device, packed weight) -> dx (cap_in, Cin); the MFMA kernel of the transposed pair cout -> cin"""
    assert (cout, cin) in S.F32_MFMA_SHAPES
    reg = _regime(rec, n_in, cap_in, cin)
    assert cap_in >= R32.full_tile_cap(cin) and reg["G"] == R32.resident(cin) and reg["full"]
    rng = np.random.default_rng(5)
    for name, draw in (("random", R32.draw32), ("integer", R32.draw32_exact)):
        d = draw(rng, 1, m, cin, cout, ksize)
        t0 = time.perf_counter()
        sums = R.dgrad(d["dy"], d["wp"], nbr, n_in)
        V, e = R32.epilogue(sums)
        if name == "integer":
            R32.assert_exactly_summable(sums)
            e = torch.zeros_like(V)
        rec.t_ref += time.perf_counter() - t0
        dx = run(_dev_nan(d["dy"], cap_out, cuda), S.pack_weight(_dev(d["w"], cuda), F32))
        assert dx.dtype == F32 and dx.shape == (cap_in, cin)
        rec.check(f"dgrad {cout}->{cin} {name}", dx, V, e, n_in, R32.tile_rows(cin))


@pytest.mark.parametrize("C,kind,order", [(16, "sheet", "rank"), (64, "mixed", "random"), (128, "sheet", "rank")])
def test_dgrad_subm(cuda, C, kind, order):
    """conv_dgrad of a SubM layer as SparseConvFunction runs it: the forward's own table, the offsets mirrored and the slabs transposed"""
    n, spare = _n_full(C), 3000
    cap = n + spare
    rec = Recorder(f"f32 dgrad subm {C}->{C} {kind}/{order} n={n} cap={cap}")
    idx, B, shape, d_idx, n_dev, grid, rb = _subm(cuda, kind, n, cap, order)
    run = lambda dy, wp: S.conv_dgrad(dy, wp.flip(0).transpose(1, 2).contiguous(), rb.nbr, n_dev, cap, pretransposed=True)
    _dgrad_case(rec, cuda, C, C, 3, n, cap, n, cap, R.neighbours_subm(idx, B, shape), run)
    rec.done()


@pytest.mark.parametrize("cin,cout", [(16, 32), (32, 64), (64, 128)])
def test_dgrad_strided(cuda, cin, cout):
    """the strided layers' data gradients: the transposed pairs 32 -> 16, 64 -> 32 and 128 -> 64 on the transposed table"""
    B, shape, density, k, s, p = STRIDED[cin, cout]
    spare = 2000
    idx, n_in, m, d_idx, n_dev, grid, rb, nbr = _strided_setup(cuda, B, shape, density, k, s, p, spare)
    rec = Recorder(f"f32 dgrad strided {cin}->{cout} n_in={n_in} n_out={m}")
    nbr_t = S.rulebook_transpose(rb, rb.out_n, n_in)
    _dgrad_case(rec, cuda, cin, cout, k, n_in, n_in, m, m + spare, nbr, lambda dy, wp: S.conv_dgrad(dy, wp, nbr_t, n_dev, n_in))
    rec.done()


# ------------------------------------------------------------------------------------------------ weight gradient
def _wgrad_n(cap, chunks):
    """about 0.6 cap, no multiple of 128, and such that the device's chunks (from n) leave trailing chunks empty"""
    j = int(0.6 * cap) // chunks // 128
    return chunks * (128 * j + 1) + 5


WGRAD = [   # (Cin, Cout, pair lists, type of x, type of dy)
    (16, 16, False, F32, F32), (64, 64, False, F32, F32), (64, 128, False, F32, F32), (128, 128, False, F32, F32),
    (5, 16, False, F32, F32), (5, 16, True, F32, F32),
    (5, 16, False, F32, torch.bfloat16), (5, 16, False, torch.bfloat16, F32), (64, 64, False, F32, torch.bfloat16), (64, 64, False, torch.bfloat16, F32),
]


@pytest.mark.parametrize("cin,cout,pairs,tx,ty", WGRAD, ids=lambda v: str(v).replace("torch.", ""))
def test_wgrad(cuda, cin, cout, pairs, tx, ty):
    """conv_wgrad in f32 and in the mixed types of conv_input under the 16-bit engines: all chunks of the shape, their borders on
    the device from n (about 0.6 of the capacity: trailing chunks empty; and n = cap - 3), both layouts, each call twice"""
    K = 27
    chunks_max = R32.wgrad_max_chunks(cin, cout)
    cap = 2048 * chunks_max + 1000
    chunks = R32.wgrad_chunks(cap, cin, cout)
    P = R32.wgrad_partials(cap, cin, cout, K, pairs)
    rec = Recorder(f"wgrad {cin}->{cout} {'pair lists' if pairs else 'table'} x {str(tx)[6:]} dy {str(ty)[6:]} cap={cap}")
    assert chunks == chunks_max and cap >= 2048 * chunks_max
    for n in (_wgrad_n(cap, chunks), cap - 3):
        rpc, live = R32.wgrad_rows_per_chunk(n, chunks), R32.wgrad_live_chunks(n, chunks)
        print(f"REGIME {rec.case} | n={n}: {chunks} chunks of {rpc} rows from n ({R32.wgrad_rows_per_chunk(cap, chunks)} from the capacity), {live} live | "
              f"PMAX {R32.wgrad_pmax(cin, cout)} | P = {P}")
        assert n % 128 and n % 16 and n < cap
        assert n == cap - 3 or (live < chunks and rpc != R32.wgrad_rows_per_chunk(cap, chunks))
        idx, B, shape, d_idx, n_dev, grid, rb = _subm(cuda, "sheet", n, cap, "rank")
        nbr = R.neighbours_subm(idx, B, shape)
        rng = np.random.default_rng(5)
        for name, draw in (("random", R32.draw32), ("integer", R32.draw32_exact)):
            d = draw(rng, n, n, cin, cout, 3)
            if name == "random":
                d["x"] = d["x"] if tx == F32 else R.round16(d["x"], tx)
                d["dy"] = d["dy"] if ty == F32 else R.round16(d["dy"], ty)
            t0 = time.perf_counter()
            sums = R.wgrad(d["x"], d["dy"], nbr)
            e = R32.wgrad_bound(sums, P).expand_as(sums.S)
            if name == "integer":
                assert float(sums.A.max()) < 2 ** 24
                e = torch.zeros_like(sums.S)
            rec.t_ref += time.perf_counter() - t0
            x, dy = _dev_nan(d["x"], cap, cuda, tx), _dev_nan(d["dy"], cap, cuda, ty)
            for module in (False, True):
                kw = dict(module_shape=(cout, 3, 3, 3, cin)) if module else {}
                dw = S.conv_wgrad(x, dy, rb, n_dev, cin, cout, pairs=pairs, **kw)
                again = S.conv_wgrad(x, dy, rb, n_dev, cin, cout, pairs=pairs, **kw)
                assert (getattr(rb, "_pairs", None) is not None) == pairs and dw.dtype == F32
                if not torch.equal(dw, again):
                    rec.fail.append(f"n={n} {name}: two runs differ in their bits")
                got = dw.reshape(cout, K, cin).permute(1, 0, 2) if module else dw
                rec.check(f"n={n} {name}{' module_shape' if module else ''}", got, sums.S, e, None, None)
    rec.done()


# ------------------------------------------------------------------------------------------------ autograd at size
def _autograd(rec, cuda, oracle, conv, cin, cout, idx, B, shape, nbr_of):
    """one autograd step of a spconv module in f32 on random and on integer data: output, data gradient and weight gradient against
    the same references as the kernels above.  nbr_of(out) -> (K, m) table over the module's output rows."""
    from findnpropagate_amd import spconv
    n_in = idx.shape[0]
    rng = np.random.default_rng(5)
    d_idx = _dev(idx, cuda)
    for name in ("random", "integer"):
        nbr = m = None
        for step in range(2 if name == "random" else 1):     # (the second step: the same bits, nothing left over from the first)
            conv.weight.grad = None
            if step == 0:
                if name == "integer":
                    conv.weight.data.copy_(_dev(rng.integers(-2, 3, tuple(conv.weight.shape)).astype(np.float32), cuda))
                w = conv.weight.detach().cpu().numpy()
                xs = (rng.standard_normal((n_in, cin)) if name == "random" else rng.integers(-2, 3, (n_in, cin))).astype(np.float32)
            x = _dev(xs, cuda).requires_grad_(True)
            out = conv(spconv.SparseConvTensor(x, d_idx, shape, B))
            if step == 0:
                nbr = nbr_of(out)
                m = nbr.shape[1]
                dys = (rng.standard_normal((m, cout)) if name == "random" else rng.integers(-2, 3, (m, cout))).astype(np.float32)
            assert out.features.shape == (m, cout) and out.features.dtype == F32
            (out.features * _dev(dys, cuda)).sum().backward()
            if step == 1:
                for what, a, b in (("out", out.features, y0), ("dx", x.grad, dx0), ("dW", conv.weight.grad, dw0)):
                    if not torch.equal(a, b):
                        rec.fail.append(f"{name}: {what} of a second step differs in its bits")
                continue
            y0, dx0, dw0 = out.features.detach().clone(), x.grad.clone(), conv.weight.grad.clone()
        K = nbr.shape[0]
        wp = np.ascontiguousarray(w.reshape(cout, K, cin).transpose(1, 0, 2))
        zero = lambda V, e: torch.zeros_like(V) if name == "integer" else e
        t0 = time.perf_counter()
        sf, sd, sw = R.conv(xs, wp, nbr), R.dgrad(dys, wp, nbr, n_in), R.wgrad(xs, dys, nbr)
        P = R32.wgrad_partials(m, cin, cout, K, False)
        refs = [("forward", y0, sf.S, R32.epilogue(sf)[1], R32.tile_rows(cout)), ("dgrad", dx0, sd.S, R32.epilogue(sd)[1], R32.tile_rows(cin)),
                ("wgrad", dw0.reshape(cout, K, cin).permute(1, 0, 2), sw.S, R32.wgrad_bound(sw, P).expand_as(sw.S), None)]
        rec.t_ref += time.perf_counter() - t0
        if name == "integer":
            assert float(sw.A.max()) < 2 ** 24
        for what, got, V, e, tile in refs:
            rec.check(f"{name} {what}", got, V, zero(V, e), None, tile)
        if name == "random":
            rows = R32.chain_rows(m, cout, R32.grid_of(m, cout), np.random.default_rng(3))
            want = R32.oracle_rows(oracle, xs, w, nbr, rows)
            bad = rows[(y0[torch.from_numpy(rows).to(cuda)].cpu().numpy() != want).any(1)]
            print(f"CHAIN {rec.case} | module forward | {rows.shape[0]} rows, {bad.shape[0]} differ")
            if bad.shape[0]:
                rec.fail.append(f"module forward: {bad.shape[0]} chosen rows are not the oracle's bits, first {bad[:12].tolist()}")


def test_autograd_subm_at_a_full_tile_size(cuda, oracle):
    from findnpropagate_amd import spconv
    C = 64
    n = _n_full(C)
    rec = Recorder(f"f32 autograd SubMConv3d {C}->{C} n={n}")
    reg = _regime(rec, n, n, C)
    assert reg["G"] == R32.resident(C) and reg["full"] and R32.wgrad_chunks(n, C, C) == 32
    idx, B, shape = sites("sheet", n, "rank")
    conv = spconv.SubMConv3d(C, C, 3, padding=1, bias=False, indice_key="a").to(cuda)
    _autograd(rec, cuda, oracle, conv, C, C, idx, B, shape, lambda out: R.neighbours_subm(idx, B, shape))
    rec.done()


def test_autograd_strided_at_a_full_tile_size(cuda, oracle):
    from findnpropagate_amd import spconv
    cin, cout = 32, 64
    B, shape, density, k, s, p = STRIDED[cin, cout]
    from test_gpu_conv_at_scale import _strided_sites
    idx = _strided_sites(B, shape, density)
    ref_out, osh, nbr = R.neighbours_strided(idx, B, shape, k, s, p)
    m = ref_out.shape[0]
    rec = Recorder(f"f32 autograd SparseConv3d {cin}->{cout} n_in={idx.shape[0]} n_out={m}")
    reg, reg_t = _regime(rec, m, m, cout), _regime(rec, idx.shape[0], idx.shape[0], cin)
    assert reg["full"] and reg["G"] == R32.resident(cout) and reg_t["full"] and reg_t["G"] == R32.resident(cin)
    conv = spconv.SparseConv3d(cin, cout, 3, stride=2, padding=1, bias=False).to(cuda)

    def nbr_of(out):
        assert list(out.spatial_shape) == osh
        return np.ascontiguousarray(nbr[:, R.match_rows(ref_out, out.indices.cpu().numpy(), osh)])

    _autograd(rec, cuda, oracle, conv, cin, cout, idx, B, shape, nbr_of)
    rec.done()
