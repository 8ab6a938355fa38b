"""The 16-bit convolution kernels (csrc/spconv.hip, spconv_tile.hip, spconv_rows128.hip, spconv_ell.hip, spconv_bwd.hip) against
the float64 reference of tests/ref64.py AT FULL-TILE SIZES: full tiles of MB blocks per wave, several rounds of the persistent
loop, the slot rotation and the XCD row split of the sorted sweep — the regime the benchmark runs them in, where every other
test compares kernels with each other only.  Every element of every row below n must lie within its own DERIVED bound (ref64's
docstring); there is no allowance.  The err / bound ratios each case prints are for the record, never a criterion.

The row counts follow from the launch geometry of csrc/spconv.hip, restated here (MfmaWg, MfmaOcc, launch_mfma_k): a workgroup
has NW waves of MB 16-row blocks, a CU holds WAVES * 4 / NW workgroups, the persistent grid has 256 of those per CU count, and
the n rows are cut into one contiguous range per workgroup — so a workgroup runs `rounds` full tiles when n reaches `rounds`
times the round size below.  Each case has n above two rounds plus a partial one, n not a multiple of 16, and spare capacity."""
import time

import numpy as np
import pytest
import torch

import ref64 as R
from findnpropagate_amd import sparse as S
from test_gpu_rows128 import _lattice, _sheet

pytestmark = pytest.mark.gpu

CUS = 256


def _nw(cin, cout):        # MfmaWg::NW
    return 8 if cin == cout and cin >= 32 else 4


def _mb(cin, cout):        # MfmaWg::MB
    return 3 if cout >= 128 else 2 if (cin == cout or (cin, cout) == (16, 32)) else 4


def _waves(cin, cout):     # MfmaOcc::WAVES
    return 2 if (cin, cout) == (128, 128) else 4 if (cin == cout or (cin, cout) == (16, 32)) else 3 if (cin < cout and cout <= 64) else 2


def tile_rows(cin, cout):
    return _nw(cin, cout) * _mb(cin, cout) * 16


def round_rows(cin, cout):
    """rows of one round of the persistent grid (launch_mfma_k: resident = 256 * (WAVES * 4 / NW) workgroups of NW * MB * 16 rows;
    the LDS limit of 160 KiB per CU does not bind for any of these layers)"""
    return CUS * (_waves(cin, cout) * 4 // _nw(cin, cout)) * tile_rows(cin, cout)


FOUR_WAVE_BELOW = CUS * 8 * 3 * 16      # 98 304: 128 -> 128, 16-bit output, 3x3x3 below this capacity runs the four-wave NWO = 4 form (launch_mfma)
ROWS128_MIN_CAP = CUS * 8 * 16          # 32 768: the sorted sweep takes the LDS-DMA row pipeline from here on (fnp_spconv_forward_sorted)
FOUR_WAVE_ROUND = CUS * 2 * 4 * 2 * 16  # 65 536: its round (two resident workgroups of 4 waves x MB_SMALL = 2 blocks)

assert round_rows(16, 16) == round_rows(16, 32) == round_rows(32, 32) == round_rows(64, 64) == 131072
assert round_rows(32, 64) == 196608 and round_rows(64, 128) == round_rows(128, 128) == FOUR_WAVE_BELOW == 98304
assert round_rows(32, 16) == round_rows(64, 32) == round_rows(128, 64) == 131072


# ------------------------------------------------------------------------------------------------ sites
def _solid(n):
    """one solid block of sites, 12 cells thick: all 27 offsets are live for most rows; rank order"""
    side = int(np.ceil(np.sqrt(n / 12.0)))
    shape = [12, side, side]
    zz, yy, xx = np.meshgrid(np.arange(12), np.arange(side), np.arange(side), indexing="ij")
    idx = np.stack([np.zeros(zz.size, np.int64), zz.ravel(), yy.ravel(), xx.ravel()], 1).astype(np.int32)
    idx = idx[np.lexsort((idx[:, 1], idx[:, 3], idx[:, 2], idx[:, 0]))][:n]
    return idx, 1, shape


_SITES = {}


def sites(kind, n, order):
    """the sheet / lattice / mixed generators of test_gpu_rows128.py with as many scenes as n needs, and the solid block;
    order 'rank' (sorted by cell as the rank grid numbers them) or 'random'"""
    k = (kind, n, order)
    if k in _SITES:
        return _SITES[k]
    rng = np.random.default_rng(4321)
    if kind == "solid":
        idx, B, shape = _solid(n)
    elif kind == "sheet":
        B, shape = n // 60000 + 1, [5, 200, 200]
        idx = _sheet(rng, B, shape)
    elif kind == "lattice":
        B, shape = n // 50000 + 1, [9, 200, 200]
        idx = np.concatenate([_lattice(b, shape) for b in range(B)])
    else:   # mixed: sheets and scenes of isolated sites
        nb = n // 110000 + 1
        B, shape = 2 * nb, [9, 200, 200]
        idx = np.concatenate([_sheet(rng, nb, shape)] + [_lattice(b, shape) for b in range(nb, 2 * nb)])
    assert idx.shape[0] >= n, (kind, n, idx.shape[0])
    idx = idx[rng.permutation(idx.shape[0])[:n]]
    if order == "rank":
        idx = idx[np.lexsort((idx[:, 1], idx[:, 3], idx[:, 2], idx[:, 0]))]
    _SITES[k] = (np.ascontiguousarray(idx), B, shape)
    return _SITES[k]


class Recorder:
    """collects the failures of a case's paths (all are reported, not the first only) and prints the worst ratio of each"""

    def __init__(self, case):
        self.case, self.fail, self.t_ref, self.t0 = case, [], 0.0, time.perf_counter()
        print()

    def check(self, path, got, V, e, n, tile):
        worst, rep = R.check(got, V, e, n, tile)
        print(f"RATIO {self.case} | {path} | {worst:.4g}")
        if rep is not None:
            self.fail.append(f"{path}: {rep}")
        return worst

    def done(self):
        print(f"TIME {self.case} | reference {self.t_ref:.1f} s | whole case {time.perf_counter() - self.t0:.1f} s")
        assert not self.fail, f"{self.case}:\n" + "\n".join(self.fail)


def _dev(a, cuda, td=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return t if td is None else t.to(td)


FORMS = [("plain", False, False, False), ("bn-relu", False, True, True), ("res-bn-relu", True, True, True), ("res", True, False, False)]


def _nan_out(cap, cout, dtype, cuda):
    return torch.full((cap, cout), float("nan"), dtype=dtype, device=cuda)


class Layer:
    """inputs of one layer on the device and its reference sums; run(fn) checks every epilogue form of one path"""

    def __init__(self, rec, cuda, td, cin, cout, ksize, rows_in, cap_in, n_out, cap_out, nbr, tile):
        rng = np.random.default_rng(99)
        self.rec, self.cuda, self.td, self.cin, self.cout, self.n, self.cap, self.tile = rec, cuda, td, cin, cout, n_out, cap_out, tile
        self.d = d = R.draw(rng, cap_in, cap_out, cin, cout, ksize, td)
        t0 = time.perf_counter()
        self.sums = R.conv(d["x"][:rows_in], d["wp"], nbr)
        rec.t_ref += time.perf_counter() - t0
        self.x, self.wp = _dev(d["x"], cuda, td), S.pack_weight(_dev(d["w"], cuda), td)
        assert np.array_equal(self.wp.float().cpu().numpy(), d["wp"])
        self.sc, self.sh = _dev(d["sc"], cuda), _dev(d["sh"], cuda)
        self.res = _dev(d["res"], cuda, td)

    def ref(self, form, out_dtype):
        _, res, scaled, relu = form
        d = self.d
        t0 = time.perf_counter()
        r = R.epilogue(self.sums, d["sc"] if scaled else None, d["sh"] if scaled else None, d["res"][:self.n] if res else None, relu, out_dtype)
        self.rec.t_ref += time.perf_counter() - t0
        return r

    def run(self, path, fn, out_dtype=None, forms=FORMS, takes_out=True):
        """fn(scale, shift, residual, relu, out) -> the output tensor"""
        od = out_dtype or self.td
        for form in forms:
            name, res, scaled, relu = form
            residual = None if not res else self.res if od == self.td else self.res.to(od)
            out = _nan_out(self.cap, self.cout, od, self.cuda) if takes_out else None
            got = fn(self.sc if scaled else None, self.sh if scaled else None, residual, relu, out)
            assert got.dtype == od and (out is None or got.data_ptr() == out.data_ptr())
            V, e = self.ref(form, od)
            self.rec.check(f"{path} {'f32 out ' if od == torch.float32 else ''}{name}", got, V, e, self.n, self.tile)


def _n_for(cin, cout, rounds=2, extra=0.17):
    """rows for `rounds` full rounds plus a partial one, not a multiple of 16"""
    r = round_rows(cin, cout)
    n = rounds * r + int(extra * r) // 16 * 16 + 5
    assert n % 16 and n > rounds * r
    return n


def _subm_setup(cuda, kind, n, spare, order):
    idx, B, shape = sites(kind, n, order)
    full = np.concatenate([idx, np.zeros((spare, 4), np.int32)]) if spare else idx
    d_idx = _dev(full, cuda)
    n_dev = S.device_scalar(n, cuda)
    grid = S.build_grid(d_idx, n_dev, B, shape)
    return idx, B, shape, d_idx, n_dev, grid


# ------------------------------------------------------------------------------------------------ 16-channel SubM layers
@pytest.mark.parametrize("td", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("cout,kind,order", [(16, "sheet", "rank"), (32, "sheet", "rank"), (16, "mixed", "random"), (32, "solid", "rank")])
def test_16_channel_layers(cuda, kind, order, cout, td):
    """16 -> 16 and 16 -> 32 on the table (the PAIR form of spconv_mfma_kernel: two offsets per matrix step), on the compact
    rulebook with the matrix kernel and with the VALU kernel."""
    cin = 16
    n, spare = _n_for(cin, cout), 3000
    idx, B, shape, d_idx, n_dev, grid = _subm_setup(cuda, kind, n, spare, order)
    cap = n + spare
    assert n >= 2 * round_rows(cin, cout) and cap > n and n % 16
    rec = Recorder(f"subm {cin}->{cout} {kind}/{order} n={n} cap={cap} {td}")
    nbr = R.neighbours_subm(idx, B, shape)
    L = Layer(rec, cuda, td, cin, cout, 3, n, cap, n, cap, nbr, tile_rows(cin, cout))
    rb = S.rulebook_subm(d_idx, n_dev, grid, 3)
    assert rb.cap_out == cap and getattr(rb, "_sorted", None) is None and getattr(rb, "_tile_rb", None) is None
    L.run("table", lambda sc, sh, r, relu, out: S.conv_forward(L.x, L.wp, rb, n_dev, scale=sc, shift=sh, residual=r, relu=relu, out=out))
    L.run("table", lambda sc, sh, r, relu, out: S.conv_forward(L.x, L.wp, rb, n_dev, scale=sc, shift=sh, residual=r, relu=relu, out=out),
          out_dtype=torch.float32, forms=FORMS[2:3])
    ell = S.rulebook_subm_ell(d_idx, n_dev, grid, pool_records=3 * cap + 8)
    assert ell._ell is not None and ell.nbr is None and (cin, cout) in S.ELL_SHAPES
    for mfma in (True, False):
        L.run(f"ell {'mfma' if mfma else 'valu'}", lambda sc, sh, r, relu, out: S.conv_forward_ell(L.x, L.wp, ell, n_dev, scale=sc, shift=sh, residual=r,
                                                                                                relu=relu, mfma=mfma), takes_out=False)
    assert int(ell._ell[2].item()) <= ell._ell[1], "the record pool was large enough"
    rec.done()


# ------------------------------------------------------------------------------------------------ 32 / 64-channel SubM layers
@pytest.mark.parametrize("td", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("C,kind,order", [(32, "sheet", "rank"), (32, "mixed", "random"), (64, "sheet", "rank"), (64, "lattice", "random"),
                                          (64, "solid", "rank")])
def test_32_and_64_channel_layers(cuda, C, kind, order, td):
    """32 -> 32 and 64 -> 64: the gather kernel, the window kernel (64 channels; on rows in random order the hint must cost speed
    only), the tile-rulebook kernel on the tile rulebook of the rulebook pass and of tile_rulebook, and the split epilogue."""
    n, spare = _n_for(C, C), 3000
    idx, B, shape, d_idx, n_dev, grid = _subm_setup(cuda, kind, n, spare, order)
    cap = n + spare
    assert n >= 2 * round_rows(C, C) and n % 16
    rec = Recorder(f"subm {C}->{C} {kind}/{order} n={n} cap={cap} {td}")
    nbr = R.neighbours_subm(idx, B, shape)
    L = Layer(rec, cuda, td, C, C, 3, n, cap, n, cap, nbr, tile_rows(C, C))
    rb = S.rulebook_subm(d_idx, n_dev, grid, 3)
    assert getattr(rb, "_tile_rb", None) is None and S.tiled_fits(cap, C, rb.nbr.shape[1], cap)
    fwd = lambda rbx, **kw: (lambda sc, sh, r, relu, out: S.conv_forward(L.x, L.wp, rbx, n_dev, scale=sc, shift=sh, residual=r, relu=relu, out=out, **kw))
    L.run("gather", fwd(rb, ranked=False, tile=False))
    L.run("gather", fwd(rb, ranked=False, tile=False), out_dtype=torch.float32, forms=FORMS[2:3])
    if C == 64:
        L.run("window", fwd(rb, ranked=True, tile=False))
    L.run("tile (tile_rulebook)", fwd(rb, ranked=True, tile=True))
    assert C in rb._tile_rb
    grid2 = S.build_grid(d_idx, n_dev, B, shape)
    rb2 = S.rulebook_subm(d_idx, n_dev, grid2, 3, tile_channels=C)
    assert C in rb2._tile_rb and not rb2._lean
    L.run("tile (rulebook pass)", fwd(rb2, ranked=True, tile=True), forms=FORMS[1:3])
    if C == 64:
        _split(L, rb, n_dev, "tiled split", dict(ranked=True, tile=True))
    rec.done()


def _split(L, rb, n_dev, path, kw):
    """conv_forward_split: y against the reference (f32 bound; the f32 residual and the 16-bit addend both enter behind the
    scale), hi + lo against y within 2^-17 |y| as its docstring promises"""
    rng = np.random.default_rng(7)
    add = R.round16(rng.standard_normal((L.cap, L.cout)).astype(np.float32), L.td)
    res32 = L.res.float()
    y, hi, lo = S.conv_forward_split(L.x, L.wp, rb, n_dev, scale=L.sc, shift=L.sh, residual=res32, addend=_dev(add, L.cuda, L.td), relu=True, **kw)
    d = L.d
    # |res + addend| <= |res| + |addend| is what the f32 additions see: two rows of the bound's last term
    t0 = time.perf_counter()
    both = d["res"][:L.n].astype(np.float64) + add[:L.n]
    V, e = R.epilogue(L.sums, d["sc"], d["sh"], both, True, torch.float32)
    e = e + 4 * 2.0 ** -24 * torch.from_numpy(np.abs(d["res"][:L.n]).astype(np.float64) + np.abs(add[:L.n]) - np.abs(both))
    L.rec.t_ref += time.perf_counter() - t0
    L.rec.check(f"{path} y", y, V, e, L.n, L.tile)
    if L.td != torch.bfloat16:    # (the promise is the bf16x3 engine's: an fp16 lo is a subnormal for |y| < 2^-3 and cannot carry the remainder)
        return
    yy = y[:L.n].double()
    ok = (hi[:L.n].double() + lo[:L.n].double() - yy).abs() <= 2.0 ** -17 * yy.abs()
    if not bool(ok.all()):
        L.rec.fail.append(f"{path}: hi + lo differs from y by more than 2^-17 |y| in {int((~ok).sum())} elements")


# ------------------------------------------------------------------------------------------------ 128 -> 128
# (kind, order, n, spare): both sides of the four-wave threshold (capacity 98 304) and of the row-pipeline threshold (32 768)
CASES_128 = [
    ("solid", "rank", 30005, 2000),                              # cap < 32 768: four-wave form; sorted: the register pipeline
    ("sheet", "rank", FOUR_WAVE_ROUND + 20005, 3000),            # cap < 98 304: four-wave form, one full round + a partial; sorted: row pipeline, a partial round
    ("sheet", "rank", FOUR_WAVE_BELOW + 16 * 500 + 5, 0),        # eight-wave form just above its threshold; row pipeline: one round
    ("sheet", "rank", _n_for(128, 128), 3000),                   # two rounds + a partial one
    ("mixed", "random", _n_for(128, 128, rounds=3, extra=0.1), 5000),   # three rounds +, isolated rows among connected ones
]


@pytest.mark.parametrize("td", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind,order,n,spare", CASES_128)
def test_128_channel_layers(cuda, kind, order, n, spare, td):
    """128 -> 128: the plain sweep (four-wave form below 98 304 rows of capacity, the eight-wave MB = 3 instance of the benchmark
    above), then the class-sorted sweep on the same rulebook (register pipeline below 32 768 rows of capacity, the LDS-DMA row
    pipeline above) — one reference for both."""
    C = 128
    idx, B, shape, d_idx, n_dev, grid = _subm_setup(cuda, kind, n, spare, order)
    cap = n + spare
    assert n % 16
    four_wave, rows128 = cap < FOUR_WAVE_BELOW, cap >= ROWS128_MIN_CAP
    rec = Recorder(f"subm 128->128 {kind}/{order} n={n} cap={cap} {td}")
    nbr = R.neighbours_subm(idx, B, shape)
    L = Layer(rec, cuda, td, C, C, 3, n, cap, n, cap, nbr, 128 if four_wave else 384)
    rb = S.rulebook_subm(d_idx, n_dev, grid, 3)
    fwd = lambda sc, sh, r, relu, out: S.conv_forward(L.x, L.wp, rb, n_dev, scale=sc, shift=sh, residual=r, relu=relu, out=out, ranked=True)
    assert getattr(rb, "_sorted", None) is None
    L.run("four-wave" if four_wave else "eight-wave", fwd)
    L.run("eight-wave", fwd, out_dtype=torch.float32, forms=FORMS[2:3])      # (an f32 output never takes the four-wave form)
    S.classsort(rb, n_dev, C)
    assert rb._sorted is not None and (cap >= ROWS128_MIN_CAP) == rows128
    L.tile = 384
    L.run("sorted row pipeline" if rows128 else "sorted register pipeline", fwd)
    if kind == "mixed":
        _split(L, rb, n_dev, "sorted split", dict(ranked=True))
    rec.done()


@pytest.mark.parametrize("td", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("cap", [40000, 150000])
def test_128_channel_thin_frames_under_a_fixed_capacity(cuda, cap, td):
    """a replayed graph's fixed capacity with a thin frame: n in {1, 17, 400} rows under 40 000 and 150 000 rows of capacity"""
    C = 128
    rec = Recorder(f"subm 128->128 thin frames cap={cap} {td}")
    for n in (1, 17, 400):
        idx, B, shape = sites("sheet", n, "rank")
        d_idx = _dev(np.concatenate([idx, np.zeros((cap - n, 4), np.int32)]), cuda)
        n_dev = S.device_scalar(n, cuda)
        rb = S.rulebook_subm(d_idx, n_dev, S.build_grid(d_idx, n_dev, B, shape), 3)
        four_wave = cap < FOUR_WAVE_BELOW
        assert cap >= ROWS128_MIN_CAP and four_wave == (cap == 40000)
        L = Layer(rec, cuda, td, C, C, 3, n, cap, n, cap, R.neighbours_subm(idx, B, shape), 384)
        fwd = lambda sc, sh, r, relu, out: S.conv_forward(L.x, L.wp, rb, n_dev, scale=sc, shift=sh, residual=r, relu=relu, out=out, ranked=True)
        L.run(f"n={n} {'four-wave' if four_wave else 'eight-wave'}", fwd, forms=FORMS[1:3])
        S.classsort(rb, n_dev, C)
        assert rb._sorted is not None
        L.run(f"n={n} sorted row pipeline", fwd, forms=FORMS[1:3])
    rec.done()


# ------------------------------------------------------------------------------------------------ strided layers
_STRIDED_IN = {}


def _strided_sites(B, shape, density):
    k = (B, tuple(shape), density)
    if k not in _STRIDED_IN:
        rng = np.random.default_rng(777)
        occ = rng.random((B, *shape)) < density
        idx = np.argwhere(occ).astype(np.int32)
        _STRIDED_IN[k] = np.ascontiguousarray(idx[rng.permutation(idx.shape[0])])     # rows in random order: the grid carries a permutation
    return _STRIDED_IN[k]


def _strided_setup(cuda, B, shape, density, k, s, p, spare):
    idx = _strided_sites(B, shape, density)
    n_in = idx.shape[0]
    out, osh, nbr = R.neighbours_strided(idx, B, shape, k, s, p)
    m = out.shape[0]
    d_idx = _dev(idx, cuda)
    n_dev = S.device_scalar(n_in, cuda)
    grid = S.build_grid(d_idx, n_dev, B, shape)
    rb = S.rulebook_strided(d_idx, n_dev, grid, k, s, p, cap_out=m + spare)
    assert int(rb.out_n.item()) == m and rb.out_shape == osh
    order = R.match_rows(out, rb.out_indices[:m].cpu().numpy(), osh)       # device row -> reference row
    return idx, n_in, m, d_idx, n_dev, grid, rb, np.ascontiguousarray(nbr[:, order])


STRIDED_VOLUME = (2, [13, 400, 398], 0.1)     # ~413 k input sites, ~0.5 M output sites: above two rounds of the widest round (32 -> 64)


@pytest.mark.parametrize("td", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("cin,cout", [(32, 64), (64, 128)])
@pytest.mark.parametrize("pad", [(1, 1, 1), (0, 1, 1)])
def test_strided_layers(cuda, cin, cout, pad, td):
    """the 3x3x3 stride-2 layers on the table and with the rulebook rows computed inside the kernel"""
    B, shape, density = STRIDED_VOLUME
    spare = 2000
    idx, n_in, m, d_idx, n_dev, grid, rb, nbr = _strided_setup(cuda, B, shape, density, 3, 2, pad, spare)
    cap = m + spare
    assert m >= 2 * round_rows(cin, cout) and m % 16, (m, round_rows(cin, cout))
    rec = Recorder(f"strided {cin}->{cout} pad={pad} n_in={n_in} n_out={m} cap={cap} {td}")
    L = Layer(rec, cuda, td, cin, cout, 3, n_in, n_in, m, cap, nbr, tile_rows(cin, cout))
    forms = [f for f in FORMS if not f[1]]        # (a strided layer has no residual)
    L.run("table", lambda sc, sh, r, relu, out: S.conv_forward(L.x, L.wp, rb, rb.out_n, scale=sc, shift=sh, relu=relu, out=out), forms=forms)
    L.run("table", lambda sc, sh, r, relu, out: S.conv_forward(L.x, L.wp, rb, rb.out_n, scale=sc, shift=sh, relu=relu, out=out), forms=forms[1:],
          out_dtype=torch.float32)
    lean = S.rulebook_strided(d_idx, n_dev, grid, 3, 2, pad, cap_out=cap, want_nbr=False)
    assert lean.nbr is None and lean.in_grid is not None and torch.equal(lean.out_indices[:m], rb.out_indices[:m])
    L.run("in-kernel rulebook", lambda sc, sh, r, relu, out: S.conv_forward_strided(L.x, L.wp, lean, scale=sc, shift=sh, relu=relu, out=out), forms=forms)
    rec.done()


@pytest.mark.parametrize("td", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_conv_out(cuda, td):
    """conv_out: (3, 1, 1) stride (2, 1, 1), 128 -> 128 — the run-time-K instance of the eight-wave kernel"""
    B, shape, density, spare = 2, [5, 250, 250], 0.6, 2000
    idx, n_in, m, d_idx, n_dev, grid, rb, nbr = _strided_setup(cuda, B, shape, density, (3, 1, 1), (2, 1, 1), 0, spare)
    assert m >= 2 * round_rows(128, 128) and m % 16, m
    rec = Recorder(f"conv_out 128->128 n_in={n_in} n_out={m} {td}")
    L = Layer(rec, cuda, td, 128, 128, (3, 1, 1), n_in, n_in, m, m + spare, nbr, 384)
    forms = [f for f in FORMS if not f[1]]
    L.run("table", lambda sc, sh, r, relu, out: S.conv_forward(L.x, L.wp, rb, rb.out_n, scale=sc, shift=sh, relu=relu, out=out), forms=forms)
    rec.done()


# ------------------------------------------------------------------------------------------------ backward
def _backward(rec, cuda, td, cin, cout, rb, n_out_dev, n_in_dev, n_in, cap_in, m, cap_out, nbr, ksize=3):
    rng = np.random.default_rng(5)
    d = R.draw(rng, cap_in, cap_out, cin, cout, ksize, td)
    x, dy = _dev(d["x"], cuda, td), _dev(d["dy"], cuda, td)
    wp = S.pack_weight(_dev(d["w"], cuda), td)
    K = nbr.shape[0]
    # data gradient: the forward kernel of the transposed channel pair on the transposed table
    t0 = time.perf_counter()
    V, e = R.epilogue(R.dgrad(d["dy"][:m], d["wp"], nbr, n_in), out_dtype=td)
    rec.t_ref += time.perf_counter() - t0
    nbr_t = S.rulebook_transpose(rb, n_out_dev, cap_in)
    dx = S.conv_dgrad(dy, wp, nbr_t, n_in_dev, cap_in)
    assert n_in >= 2 * round_rows(cout, cin), (n_in, round_rows(cout, cin))
    rec.check(f"dgrad {cout}->{cin}", dx, V, e, n_in, tile_rows(cout, cin))
    # weight gradient, on the pair lists and on the table, and in the module's layout
    t0 = time.perf_counter()
    V, e = R.epilogue(R.wgrad(d["x"][:n_in], d["dy"][:m], nbr))
    rec.t_ref += time.perf_counter() - t0
    assert (cin, cout) in S.WGRAD_PAIR_SHAPES
    for pairs in (True, False):
        dw = S.conv_wgrad(x, dy, rb, n_out_dev, cin, cout, pairs=pairs)
        assert (getattr(rb, "_pairs", None) is not None) == pairs or not pairs
        rec.check(f"wgrad {'pair lists' if pairs else 'table'}", dw, V, e, None, None)
    kk = R._triple(ksize)
    dwm = S.conv_wgrad(x, dy, rb, n_out_dev, cin, cout, pairs=True, module_shape=(cout, *kk, cin))
    rec.check("wgrad module_shape", dwm.reshape(cout, K, cin).permute(1, 0, 2), V, e, None, None)
    # integer inputs: every partial sum is an integer below 2^24, f32 adds them exactly in any grouping — the bound is ZERO, and
    # a single lost pair (or a lost chunk tail, which the rounding bound above is too wide for at this size) shows
    z = R.draw_exact(rng, cap_in, cap_out, cin, cout, td)
    t0 = time.perf_counter()
    sums = R.wgrad(z["x"][:n_in], z["dy"][:m], nbr)
    rec.t_ref += time.perf_counter() - t0
    assert float(sums.A.max()) < 2 ** 24
    zx, zdy = _dev(z["x"], cuda, td), _dev(z["dy"], cuda, td)
    for pairs in (True, False):
        dw = S.conv_wgrad(zx, zdy, rb, n_out_dev, cin, cout, pairs=pairs)
        rec.check(f"wgrad exact {'pair lists' if pairs else 'table'}", dw, sums.S, torch.zeros_like(sums.S), None, None)


@pytest.mark.parametrize("td", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("C,kind,order", [(16, "sheet", "rank"), (64, "mixed", "random"), (128, "sheet", "rank")])
def test_subm_backward(cuda, C, kind, order, td):
    """conv_dgrad (the forward kernel on rulebook_transpose) and conv_wgrad of the SubM layers at two rounds and more"""
    n, spare = _n_for(C, C), 3000
    idx, B, shape, d_idx, n_dev, grid = _subm_setup(cuda, kind, n, spare, order)
    cap = n + spare
    rec = Recorder(f"backward subm {C}->{C} {kind}/{order} n={n} cap={cap} {td}")
    rb = S.rulebook_subm(d_idx, n_dev, grid, 3)
    _backward(rec, cuda, td, C, C, rb, n_dev, n_dev, n, cap, n, cap, R.neighbours_subm(idx, B, shape))
    rec.done()


@pytest.mark.parametrize("td", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("cin,cout", [(16, 32), (32, 64), (64, 128)])
def test_strided_backward(cuda, cin, cout, td):
    """the strided layers' gradients: the data gradient runs the transposed pairs 32 -> 16, 64 -> 32 and 128 -> 64"""
    B, shape, density = STRIDED_VOLUME
    spare = 2000
    idx, n_in, m, d_idx, n_dev, grid, rb, nbr = _strided_setup(cuda, B, shape, density, 3, 2, 1, spare)
    rec = Recorder(f"backward strided {cin}->{cout} n_in={n_in} n_out={m} {td}")
    _backward(rec, cuda, td, cin, cout, rb, rb.out_n, n_dev, n_in, n_in, m, m + spare, nbr)
    rec.done()
