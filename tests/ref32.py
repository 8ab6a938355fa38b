"""What float32 INPUTS change in the reference of tests/ref64.py: the bound, the inputs, the C oracle's fmaf chain on chosen rows,
and the launch geometry of the f32 kernels restated as pure functions.  Everything that does not depend on the type — neighbour
tables from coordinates, Sums, conv / dgrad / wgrad, check / assert_within — is ref64's and is used as it is.  A helper module.

THE BOUND.  S = sum x*w over the terms that exist, A = sum |x|*|w| over the same terms, T = the number of terms, as in ref64.
With f32 inputs a product is NOT exact in f32, but no kernel here ever forms one on its own: every term enters through an fmaf or
through v_mfma_f32_16x16x4_f32, which is, bit for bit, a k-ordered chain of fmaf (csrc/spconv_f32.hip) — one rounding per term.
A partial sum that is later added to another (the chunk partials of a weight gradient, the group sums inside a workgroup, the
lanes of a butterfly) costs one more rounding per addition; an addition of zero (an empty chunk, the zero an accumulator starts
from, fmaf(0, w, acc) for an absent neighbour) is exact and may be counted or not.  So a sum of T terms evaluated with T fused
multiply-adds and P further additions, IN ANY ORDER AND GROUPING, is the exact sum of the terms each multiplied by at most T + P
factors (1 + d), |d| <= u = 2^-24, and errs by at most (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1)

    gamma * A,    gamma = (T + P) * u / (1 - (T + P) * u).

P = 0 for the forward and the data gradient (one chain per output element).  For a weight gradient P is the number of partial
results that are added: the row chunks of wgrad_partial_kernel (`wgrad_chunks`), and for the few-pairs kernel (5 -> 16) the group
sums of a workgroup and the lanes of the reduction as well — `wgrad_partials` counts them from the launch code, and counts
generously, which is safe: the bound holds for every T' <= T + P.
ASSUMPTIONS: round to nearest in every fmaf and addition; no denormal inputs and no underflow (the inputs drawn here have none, and
the matrix unit's treatment of denormals does not enter); the f32 matrix instruction being that fmaf chain.
Nothing about the order of the chain enters, and no constant here was set by looking at a result of the GPU.

The epilogue V = relu?(S * scale + shift + residual) is ref64.epilogue's with this gamma: |scale| * gamma * A for the scaled
accumulator, 4 * 2^-24 * (|S * scale| + |shift| + |residual|) for its at most three f32 operations (a contracted fma omits one),
and for a 16-bit output — conv_input under the 16-bit engines — one rounding u16 * (|V| + e) plus 2^-25 for fp16 subnormals.

INTEGER INPUTS (draw32_exact).  x, w, dy, residual, scale and shift are small integers, so that every partial sum of every order
is an integer below 2^24 and every f32 operation on it is exact: forward, both gradients and the whole epilogue must then equal the
float64 reference BIT FOR BIT ON EVERY ROW.  That is what shows one lost pair in a weight gradient, whose rounding bound at
2 * 10^5 pairs is wider than the whole contribution of a pair.  A 16-bit output is the exact value rounded once (`exact16`).

THE CHAIN.  The f32 forward kernels claim more than a bound: the oracle's k-ascending, cin-ascending fmaf chain, bit for bit.
`oracle_rows` hands oracle.conv_apply the pairs of a CHOSEN SUBSET of output rows, made from ref64's coordinate-derived table
(ascending k, output rows renumbered), and returns the oracle's f32 result for those rows; `chain_rows` chooses the rows from the
restated geometry: the first and last 16 rows of the first, the last and some middle workgroup ranges and of the ranges on both
sides of every XCD border of the range split, the rows around every tile and wave border inside those ranges, the last partial
block, and about a thousand random rows."""
import numpy as np
import torch

import ref64 as R

U = 2.0 ** -24                # unit roundoff of f32, round to nearest


def gamma(T, P=0):
    t = (T + P) * U
    return t / (1.0 - t)


def epilogue(sums, scale=None, shift=None, residual=None, relu=False, out_dtype=torch.float32, P=0):
    """(V, bound) float64 tensors: ref64.epilogue with the gamma of this module (see the docstring)"""
    S, A = sums.S, sums.A
    f = lambda v: None if v is None else torch.as_tensor(np.asarray(v), dtype=torch.float64)
    scale, shift, residual = f(scale), f(shift), f(residual)
    sc = scale if scale is not None else torch.ones((), dtype=torch.float64)
    V = S * sc
    mag = V.abs()
    if shift is not None:
        V = V + shift
        mag = mag + shift.abs()
    if residual is not None:
        V = V + residual
        mag = mag + residual.abs()
    e = sc.abs() * gamma(sums.T, P) * A
    if scale is not None or residual is not None:
        e = e + 4 * U * mag
    if relu:
        V = V.clamp_min(0.0)
    if out_dtype != torch.float32:
        e = e + R.U16[out_dtype] * (V.abs() + e)
        if out_dtype == torch.float16:
            e = e + R.FP16_SUBNORMAL
    return V, e


def exact16(V, td):
    """an exactly known value (an integer below 2^24) stored in the 16-bit type: one rounding to nearest even"""
    return torch.as_tensor(V).to(torch.float32).to(td)


# ------------------------------------------------------------------------------------------------ inputs
def _pack(w, k):
    Cout, Cin = w.shape[0], w.shape[-1]
    return np.ascontiguousarray(w.reshape(Cout, k[0] * k[1] * k[2], Cin).transpose(1, 0, 2))


def draw32(rng, rows_in, rows_out, Cin, Cout, ksize):
    """f32 normal data that is NOT rounded to 16 bits (no denormals: a normal deviate below 2^-126 is not drawn): x, w in the
    module layout (Cout, kD, kH, kW, Cin) and wp packed (K, Cout, Cin), BatchNorm scale / shift, residual res, gradient dy"""
    k = R._triple(ksize)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    w = f(Cout, *k, Cin) * np.float32(0.05)
    d = dict(x=f(rows_in, Cin), w=w, wp=_pack(w, k), sc=rng.uniform(0.5, 1.5, Cout).astype(np.float32), sh=f(Cout), res=f(rows_out, Cout),
             dy=f(rows_out, Cout))
    for v in d.values():
        assert not ((v != 0) & (np.abs(v) < 2.0 ** -126)).any()
    return d


def draw32_exact(rng, rows_in, rows_out, Cin, Cout, ksize):
    """the same fields as small integers: x, w, dy in -2 .. 2, residual and shift in -3 .. 3, scale in 1 .. 3"""
    k = R._triple(ksize)
    i = lambda lo, hi, *s: rng.integers(lo, hi + 1, s).astype(np.float32)
    w = i(-2, 2, Cout, *k, Cin)
    return dict(x=i(-2, 2, rows_in, Cin), w=w, wp=_pack(w, k), sc=i(1, 3, Cout), sh=i(-3, 3, Cout), res=i(-3, 3, rows_out, Cout),
                dy=i(-2, 2, rows_out, Cout))


def assert_exactly_summable(sums, scale_max=3.0, extra=6.0):
    """every partial sum of the integer inputs, in any order, and the epilogue on top of it stay below 2^24"""
    assert float(sums.A.max()) * scale_max + extra < 2 ** 24, float(sums.A.max())


# ------------------------------------------------------------------------------------------------ the oracle's chain on chosen rows
def subset_pairs(nbr, rows):
    """pair lists (pin, pout, pn) of the output rows `rows` of a (K, n) neighbour table, offsets ascending, the output rows
    renumbered 0 .. len(rows) - 1 in the order given"""
    rows = np.asarray(rows, dtype=np.int64)
    K, m = nbr.shape[0], rows.shape[0]
    sub = nbr[:, rows]
    pin = np.zeros((K, max(m, 1)), np.int32)
    pout = np.zeros((K, max(m, 1)), np.int32)
    pn = np.zeros((K,), np.int32)
    for k in range(K):
        o = np.nonzero(sub[k] >= 0)[0]
        pn[k] = o.shape[0]
        pin[k, :o.shape[0]] = sub[k, o]
        pout[k, :o.shape[0]] = o
    return pin, pout, pn


def oracle_rows(oracle, x, w, nbr, rows, scale=None, shift=None, residual=None, relu=False):
    """the oracle's f32 result (conv_apply, then scale_shift_act when any epilogue term is given) for the output rows `rows` only;
    w in the module layout, residual over ALL output rows"""
    rows = np.asarray(rows, dtype=np.int64)
    y = oracle.conv_apply(x, w, *subset_pairs(nbr, rows), rows.shape[0])
    if scale is not None or residual is not None or relu:
        y = oracle.scale_shift_act(y, scale, shift, None if residual is None else np.ascontiguousarray(residual[rows]), relu=relu)
    return y


# ------------------------------------------------------------------------------------------------ geometry of csrc/spconv_f32.hip
def mb(cout):                 # launch_f32: 16-row blocks per wave
    return 4 if cout <= 64 else 3


def waves(cout):              # F32Occ::WAVES
    return 4 if cout <= 32 else 2


def tile_rows(cout):          # a workgroup tile: 4 waves x MB blocks x 16 rows
    return 4 * mb(cout) * 16


def resident(cout):           # the persistent grid
    return 256 * waves(cout)


def full_tile_cap(cout):
    return resident(cout) * tile_rows(cout)


def grid_of(cap, cout):
    tiles, fine = -(-cap // tile_rows(cout)), -(-cap // 64)
    return resident(cout) if tiles >= resident(cout) else min(fine, resident(cout))


def xcd_first(G):
    """the first range index of each of the eight XCDs (workgroup b runs range xcd_first[b & 7] + (b >> 3))"""
    per, rem = G >> 3, G & 7
    return [x * (per + 1) if x < rem else rem * (per + 1) + (x - rem) * per for x in range(8)]


def range_of_block(b, G):
    return xcd_first(G)[b & 7] + (b >> 3)


def ranges(n, G):
    """[row_begin, row_end) of every range 0 .. G - 1 (int64 arrays): whole 16-row blocks, balanced"""
    nblk = (n + 15) >> 4
    r = np.arange(G + 1, dtype=np.int64)
    cut = (nblk * r // G) << 4
    return cut[:-1], np.minimum(n, cut[1:])


def wave_plan(b, e, cout):
    """what the four waves of a workgroup do with the range [b, e): (small, bpw, [(rows of wave w as a list of (first, last + 1))])
    — small: the range is shorter than a tile and is cut evenly, bpw blocks per wave, one pass; else the persistent loop in steps
    of a tile, MB blocks per wave, clamped at e"""
    MB, tile = mb(cout), tile_rows(cout)
    nblk = (e - b + 15) >> 4
    small, bpw = nblk < 4 * MB, (nblk + 3) // 4
    plan = []
    for w in range(4):
        if small:
            t0 = b + w * bpw * 16
            end = min(e, t0 + bpw * 16)
            plan.append([(t0, end)] if t0 < end else [])
        else:
            plan.append([(t, min(e, t + MB * 16)) for t in range(b + w * MB * 16, e, tile)])
    return small, bpw, plan


def chain_rows(n, cout, G, rng, random_rows=1000, middle=3):
    """the rows of the chain check (sorted, unique): see the module docstring"""
    rb, re = ranges(n, G)
    live = np.nonzero(re > rb)[0]
    pick = {int(live[0]), int(live[-1])} | {int(v) for v in live[np.linspace(0, live.shape[0] - 1, middle + 2).astype(int)[1:-1]]}
    for f in xcd_first(G)[1:]:
        pick |= {r for r in (f - 1, f) if 0 <= r < G and re[r] > rb[r]}
    rows = [np.arange(n // 16 * 16 if n % 16 else max(0, n - 16), n)]
    for r in sorted(pick):
        b, e = int(rb[r]), int(re[r])
        rows += [np.arange(b, min(e, b + 16)), np.arange(max(b, e - 16), e)]
        for spans in wave_plan(b, e, cout)[2]:
            for t0, t1 in spans:
                rows += [np.arange(max(b, t0 - 2), min(e, t0 + 2)), np.arange(max(b, t1 - 2), min(e, t1 + 2))]
    rows.append(rng.integers(0, n, min(random_rows, n)))
    rows = np.unique(np.concatenate(rows))
    assert rows.min() >= 0 and rows.max() < n
    return rows


def rows_around(n, borders, rng, random_rows=1000):
    """first and last 16 rows, four rows around every border, random rows: the kernels that stride over the rows by a fixed step"""
    rows = [np.arange(0, min(16, n)), np.arange(max(0, n - 16), n), rng.integers(0, n, min(random_rows, n))]
    rows += [np.arange(max(0, b - 2), min(n, b + 2)) for b in borders if 0 < b < n]
    return np.unique(np.concatenate(rows))


# class sort of the f32 sweep (f32_classsort_kernel): one 1024-thread workgroup per range, q consecutive rows per thread
SORT_THREADS, SORT_Q_MAX = 1024, 16


def sort_q(n, G):
    rb, re = ranges(n, G)
    return -(-(re - rb) // SORT_THREADS)


def zclass(nbr):
    """class of every row of a 27-offset table: 0 no neighbour in either adjacent z plane, 1 above only (offsets 18 .. 26), 2 both,
    3 below only (offsets 0 .. 8)"""
    lo, hi = (nbr[0:9] >= 0).any(0), (nbr[18:27] >= 0).any(0)
    return np.where(lo, np.where(hi, 2, 3), np.where(hi, 1, 0))


def check_perm(perm, cls, n, G):
    """perm (n,) of the class sort against the restated ranges: a permutation of exactly each range's rows; classes ascend with no
    descent inside a range; rows of a class keep their order; a range of more than 16 * 1024 rows keeps its own order.
    AssertionError otherwise."""
    perm = np.asarray(perm).astype(np.int64)
    assert perm.shape == (n,) and perm.min() >= 0 and perm.max() < n, "perm has entries outside the rows"
    rb, re = ranges(n, G)
    rid = np.searchsorted(re, np.arange(n), side="right")            # range of a position (empty ranges have rb == re)
    assert (rb[rid] <= np.arange(n)).all() and (np.arange(n) < re[rid]).all()
    assert np.array_equal(np.sort(perm), np.arange(n)), "perm is not a permutation of the rows"
    assert np.array_equal(rid[perm], rid), "perm moves a row out of its workgroup range"
    long_ = (re - rb > SORT_THREADS * SORT_Q_MAX)[rid]
    assert np.array_equal(perm[long_], np.arange(n)[long_]), "a range too long to sort does not keep its order"
    c = cls[perm]
    inside = (np.diff(rid) == 0) & ~long_[1:]
    assert not (inside & (np.diff(c) < 0)).any(), "a class descends inside a range"
    assert (np.diff(perm)[inside & (np.diff(c) == 0)] > 0).all(), "rows of a class do not keep their order"


# first layer (spconv_first_kernel) and thread-per-element chain (spconv_valu_kernel): grid-stride rounds
FIRST_ROUND_ROWS = 2048 * 256          # launch_first: at most 2048 workgroups of 256 rows


def valu_round_elements(cap, cout):    # launch_valu: at most 4096 workgroups of 256 (row, cout) elements
    return min(-(-cap * cout // 256), 4096) * 256


# ------------------------------------------------------------------------------------------------ geometry of csrc/spconv_bwd.hip
def wgrad_max_chunks(cin, cout):
    return 128 if cin * cout <= 128 else 32 if cin * cout <= 8192 else 24


def wgrad_chunks(cap, cin, cout):
    return max(1, min(-(-cap // 2048), wgrad_max_chunks(cin, cout)))


def wgrad_rows_per_chunk(rows, chunks):
    """rows of a chunk: the HOST's from the capacity (unused by the kernels), the DEVICE's from n — the borders that count"""
    return (-(-rows // chunks) + 127) // 128 * 128


def wgrad_live_chunks(n, chunks):
    return -(-n // wgrad_rows_per_chunk(n, chunks))


def wgrad_pmax(cin, cout):
    """accumulators per thread of wgrad_partial_kernel (0: the few-pairs kernel, one)"""
    p = cin * cout
    return 0 if p <= 128 else 4 if p <= 1024 else 16 if p <= 4096 else 64


def wgrad_partials(cap, cin, cout, K, pairs):
    """P of the bound: partial results added into one element of the weight gradient.  wgrad_partial_kernel: one per chunk
    (wgrad_reduce_kernel adds them to zero in turn).  The few-pairs kernel adds the G = 256 / (Cin Cout) group sums of a workgroup
    first; on pair lists an offset may own up to all chunks * K workgroups, and the reduction adds them in eight lanes and a
    three-step butterfly."""
    chunks = wgrad_chunks(cap, cin, cout)
    if wgrad_pmax(cin, cout):
        return chunks
    G = 256 // (cin * cout)
    return (chunks * K if pairs else chunks) * (G + 1) + 8 + 3


def wgrad_bound(sums, P):
    return gamma(sums.T, P) * sums.A
