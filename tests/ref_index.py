"""A plain numpy reference of the INDEX machinery — rank grid words, rank order, neighbour tables, strided output sites — worked
out from COORDINATES alone, restating the comments of csrc/rankgrid.h and csrc/voxelize.hip, never their code paths.  int64
throughout and SPARSE: cells are looked up through sorted linear keys and np.searchsorted (the dense table of ref64._lookup
would need 8.6 GB at 12 scenes of the 41 x 1440 x 1440 grid).  A helper module, not a fixture; everything here is exact integer
work, so the comparators at the end know no tolerance.

THE RANK GRID (rankgrid.h).  A (B, D, H, W) cell grid is cut into 4 x 4 x 4 blocks; 8 x 8 blocks of the (H, W) plane form a
patch (bh, bw rounded UP to whole patches: th, tw); blocks are numbered scene, then patch row-major in (H, W), then the 64
block columns of a patch along a Z-order curve  col = (m3(by & 7) << 1) | m3(bx & 7)  (m3: bits abc -> 0a0b0c), then the
blocks of a column bottom to top:

    block = (((b * th + ty) * tw + tx) * 64 + col) * bd + bz          bit = (z & 3) * 16 + (y & 3) * 4 + (x & 3)

bits[block] is the u64 occupancy, summary[i] bit j says bits[64 i + j] != 0, base[block] is the number of occupied cells in
blocks < block (defined on occupied blocks only) and rank(cell) = base[block] + popcount(bits[block] below bit): ranks run
through the cells in ascending (block, bit).  perm maps rank -> row for tensors in another row order.

THE PREFIX SPLIT (fnp_rg_wpw).  The prefix works on UNITS of wpw summary words — 1 below 2^15 summary words, 8 from 2^15 on,
16 from 2^18 on —, groups of 64 units and chunks of 1024 units; wpw / units / chunks restate that, and the GPU cases assert
from them which form they reached."""
import numpy as np

GRID_STRIDE_ROWS = 2048 * 256     # fnp_grid_for: at most 2 048 workgroups of 256 rows, so row 524 288 opens a second round
MARK_TAB_SLOTS = 512              # rankgrid.h kMarkTab: (block, bits) pairs a workgroup's LDS table holds
CNT_TAB_SLOTS = 32                # rankgrid.h kCntTab: units a workgroup's count table holds
SCAN_TILE = 4096                  # scan.hip: points per scan tile; partial_scan_kernel scans 256 tile sums per round
SCENE_ROUND = 64                  # vox_scene_kernel: scenes per round of its one wave


def _triple(v):
    return [int(v)] * 3 if np.isscalar(v) else [int(x) for x in v]


def _m3(v):
    return (v & 1) | ((v & 2) << 1) | ((v & 4) << 2)


def _unm3(m):
    return (m & 1) | ((m >> 1) & 2) | ((m >> 2) & 4)


def dims(B, shape):
    """fnp_make_dims: blocks per axis, patches per H / W axis, number of blocks and of summary words"""
    D, H, W = (int(v) for v in shape)
    bd, bh, bw = (D + 3) // 4, (H + 3) // 4, (W + 3) // 4
    th, tw = (bh + 7) // 8, (bw + 7) // 8
    nblk = int(B) * th * tw * 64 * bd
    return dict(B=int(B), D=D, H=H, W=W, bd=bd, bh=bh, bw=bw, th=th, tw=tw, nblk=nblk, nsum=(nblk + 63) // 64)


def block_and_bit(idx, B, shape):
    """(block, bit) int64 of every row of idx (n, 4) [b, z, y, x]"""
    g = dims(B, shape)
    idx = np.asarray(idx).astype(np.int64).reshape(-1, 4)
    b, z, y, x = idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]
    by, bx = y >> 2, x >> 2
    col = (_m3(by & 7) << 1) | _m3(bx & 7)
    blk = (((b * g["th"] + (by >> 3)) * g["tw"] + (bx >> 3)) * 64 + col) * g["bd"] + (z >> 2)
    bit = ((z & 3) << 4) | ((y & 3) << 2) | (x & 3)
    return blk, bit


def block_origin(blk, B, shape):
    """the inverse numbering: (b, z0, y0, x0) of the block's first cell and whether the block lies inside the grid at all (the
    blocks of a partly filled last patch beyond H or W exist in the numbering but hold no cell)"""
    g = dims(B, shape)
    blk = np.asarray(blk).astype(np.int64)
    bz, r = blk % g["bd"], blk // g["bd"]
    col, r = r & 63, r >> 6
    tx, r = r % g["tw"], r // g["tw"]
    ty, b = r % g["th"], r // g["th"]
    by, bx = (ty << 3) | _unm3(col >> 1), (tx << 3) | _unm3(col)
    org = np.stack([b, bz << 2, by << 2, bx << 2], -1)
    ok = (blk >= 0) & (b < g["B"]) & (org[..., 2] < g["H"]) & (org[..., 3] < g["W"])
    return org, ok


def popcount(a):
    a = np.ascontiguousarray(np.asarray(a).astype(np.uint64))
    return np.unpackbits(a.view(np.uint8).reshape(-1, 8), axis=1).sum(1).astype(np.int64)


def rank_key(idx, B, shape):
    blk, bit = block_and_bit(idx, B, shape)
    return blk * 64 + bit


class Words:
    """the words of a grid on its occupied blocks: blocks (ascending ids), bits (u64), base, sum_ids / sum_words (the
    non-zero summary words), total"""

    def __init__(self, blocks, bits, base, sum_ids, sum_words, total):
        self.blocks, self.bits, self.base, self.sum_ids, self.sum_words, self.total = blocks, bits, base, sum_ids, sum_words, total


def grid_words(idx, B, shape):
    key = np.unique(rank_key(idx, B, shape))
    blocks, start = np.unique(key >> 6, return_index=True)
    one = np.left_shift(np.uint64(1), (key & 63).astype(np.uint64))
    bits = np.bitwise_or.reduceat(one, start) if key.size else np.zeros(0, np.uint64)
    cnt = popcount(bits)
    base = np.cumsum(cnt) - cnt
    sum_ids, sstart = np.unique(blocks >> 6, return_index=True)
    sone = np.left_shift(np.uint64(1), (blocks & 63).astype(np.uint64))
    sum_words = np.bitwise_or.reduceat(sone, sstart) if blocks.size else np.zeros(0, np.uint64)
    return Words(blocks, bits, base, sum_ids, sum_words, int(key.size))


def rank_order(idx, B, shape):
    """perm (n,) int64: perm[rank] = row — the rows sorted by (block, bit)"""
    return np.argsort(rank_key(idx, B, shape), kind="stable")


def rank_of(idx, B, shape):
    """rank of every row (the inverse of rank_order)"""
    o = rank_order(idx, B, shape)
    r = np.empty_like(o)
    r[o] = np.arange(o.shape[0])
    return r


class _Lookup:
    """row of a cell through sorted linear keys"""

    def __init__(self, idx, shape):
        self.shape = [int(v) for v in shape]
        self.key = self.lin(idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3])
        self.order = np.argsort(self.key, kind="stable")
        self.sorted = self.key[self.order]

    def lin(self, b, z, y, x):
        D, H, W = self.shape
        return ((b * D + z) * H + y) * W + x

    def find(self, b, z, y, x):
        D, H, W = self.shape
        ok = (z >= 0) & (z < D) & (y >= 0) & (y < H) & (x >= 0) & (x < W)
        k = self.lin(b, z, y, x)
        pos = np.minimum(np.searchsorted(self.sorted, k), max(self.sorted.shape[0] - 1, 0))
        hit = ok & (self.sorted[pos] == k) if self.sorted.size else np.zeros(k.shape, bool)
        return np.where(hit, self.order[pos] if self.sorted.size else 0, -1)


def _offsets(k):
    return [(a, b, c) for a in range(k[0]) for b in range(k[1]) for c in range(k[2])]


def neighbours_subm(idx, B, shape, ksize=3):
    """(K, n) int64: the row at coordinate + (offset - ksize // 2), or -1.  Offset k = (kz * kH + ky) * kW + kx."""
    idx = np.asarray(idx).astype(np.int64).reshape(-1, 4)
    k = _triple(ksize)
    lut = _Lookup(idx, shape)
    s = idx[lut.order]      # (the rows in key order: the keys asked for ascend with them, which np.searchsorted likes)
    nbr = np.empty((k[0] * k[1] * k[2], idx.shape[0]), np.int64)
    for j, (a, b, c) in enumerate(_offsets(k)):
        nbr[j, lut.order] = lut.find(s[:, 0], s[:, 1] + a - k[0] // 2, s[:, 2] + b - k[1] // 2, s[:, 3] + c - k[2] // 2)
    return nbr


def out_shape_of(shape, ksize, stride, padding):
    k, s, p = _triple(ksize), _triple(stride), _triple(padding)
    return [(shape[d] + 2 * p[d] - k[d]) // s[d] + 1 for d in range(3)]


def outputs_of(idx, shape, ksize, stride, padding):
    """per kernel offset: (ok (n,) bool, out (n, 4)) — the output site input row i feeds through that offset, where there is one"""
    idx = np.asarray(idx).astype(np.int64).reshape(-1, 4)
    k, s, p = _triple(ksize), _triple(stride), _triple(padding)
    osh = out_shape_of(shape, k, s, p)
    res = []
    for off in _offsets(k):
        num = [idx[:, 1 + d] + p[d] - off[d] for d in range(3)]
        ok = np.ones(idx.shape[0], bool)
        for d in range(3):
            ok &= (num[d] % s[d] == 0) & (num[d] >= 0) & (num[d] // s[d] < osh[d])
        res.append((ok, np.stack([idx[:, 0]] + [num[d] // s[d] for d in range(3)], 1)))
    return res, osh


def output_blocks(idx, B, shape, ksize, stride, padding):
    """(n, K) int64: the OUTPUT grid's block each input row marks through each offset, or -1 (what a marking workgroup puts
    into its LDS table)"""
    res, osh = outputs_of(idx, shape, ksize, stride, padding)
    return np.stack([np.where(ok, block_and_bit(o, B, osh)[0], -1) for ok, o in res], 1)


def neighbours_strided(idx, B, shape, ksize, stride, padding):
    """Output sites IN RANK ORDER OF THE OUTPUT GRID (n_out, 4) int32, the output shape and nbr (K, n_out) int64: the input row
    at out * stride - padding + offset, or -1.  An output site exists where at least one input falls into its window."""
    idx = np.asarray(idx).astype(np.int64).reshape(-1, 4)
    k, s, p = _triple(ksize), _triple(stride), _triple(padding)
    res, osh = outputs_of(idx, shape, k, s, p)
    cand = np.concatenate([o[ok] for ok, o in res]) if idx.shape[0] else np.zeros((0, 4), np.int64)
    _, first = np.unique(rank_key(cand, B, osh), return_index=True)     # ascending (block, bit) = rank order
    out = cand[first]
    lut = _Lookup(idx, shape)
    nbr = np.stack([lut.find(out[:, 0], out[:, 1] * s[0] - p[0] + a, out[:, 2] * s[1] - p[1] + b, out[:, 3] * s[2] - p[2] + c)
                    for a, b, c in _offsets(k)]) if out.shape[0] else np.zeros((k[0] * k[1] * k[2], 0), np.int64)
    return out.astype(np.int32), osh, nbr


def row_masks(nbr):
    """bit k set iff nbr[k, o] >= 0 (K <= 32), as int64"""
    K = nbr.shape[0]
    assert K <= 32
    return ((nbr >= 0).astype(np.int64) << np.arange(K, dtype=np.int64)[:, None]).sum(0)


# ------------------------------------------------------------------------------------------------ the prefix split
def wpw(nsum):
    return 16 if nsum >= (1 << 18) else 8 if nsum >= (1 << 15) else 1


def units(nsum):
    w = wpw(nsum)
    return (nsum + w - 1) // w


def chunks(nsum):
    return (units(nsum) + 1023) // 1024


def groups(nsum):
    return (units(nsum) + 63) // 64


def unit_of(blk, nsum):
    return (np.asarray(blk).astype(np.int64) >> 6) // wpw(nsum)


def counter_words(nsum):
    """the counter words a grid's unit size uses: units | groups | chunks"""
    return units(nsum) + groups(nsum) + chunks(nsum)


def workgroup_table_load(block_ids, unit_ids, group=256):
    """for consecutive `group`-row workgroups: (distinct blocks, distinct units) a workgroup puts into its LDS tables.
    block_ids / unit_ids: (n,) or (n, m) with -1 for "none"."""
    blk = np.asarray(block_ids).astype(np.int64).reshape(len(block_ids), -1)
    un = np.asarray(unit_ids).astype(np.int64).reshape(len(unit_ids), -1)
    nb, nu = [], []
    for r0 in range(0, blk.shape[0], group):
        b = np.unique(blk[r0:r0 + group])
        u = np.unique(un[r0:r0 + group])
        nb.append(int((b >= 0).sum()))
        nu.append(int((u >= 0).sum()))
    return np.array(nb), np.array(nu)


# ------------------------------------------------------------------------------------------------ the voxeliser's first-come order
def first_flags(cell_keys):
    """flag (n,) int64: point i is the first point of its cell (cell key -1: out of range, never first)"""
    k = np.asarray(cell_keys).astype(np.int64)
    valid = np.nonzero(k >= 0)[0]
    _, first = np.unique(k[valid], return_index=True)     # (np.unique: the first occurrence = the smallest point index)
    flag = np.zeros(k.shape[0], np.int64)
    flag[valid[first]] = 1
    return flag


def rows_from_scan(flag, fc, total, offsets, max_voxels):
    """voxelize.hip steps 4-5 from the exclusive scan fc of the first-point flags (total = their sum): voxels are numbered in
    the order of their first point, scene after scene, each scene cut at max_voxels.  -> (row of every point's voxel, or -1
    where the point is not a first point or its voxel is cut; first output row of every scene; kept voxels per scene)"""
    offsets = np.asarray(offsets).astype(np.int64)
    n, B = flag.shape[0], offsets.shape[0] - 1
    fc_end = np.concatenate([fc, [total]])
    start = fc_end[offsets[:-1]]
    count = np.minimum(fc_end[offsets[1:]] - start, max_voxels)
    out_base = np.cumsum(count) - count
    scene = np.minimum(np.searchsorted(offsets[1:], np.arange(n), side="right"), B - 1)
    srank = fc - start[scene]
    row = np.where((flag == 1) & (srank < max_voxels), out_base[scene] + srank, -1)
    return row, out_base, count


def first_come(cell_keys, offsets, max_voxels):
    """the voxeliser's row order from the per-point cell keys and the scene offsets"""
    flag = first_flags(cell_keys)
    return rows_from_scan(flag, np.cumsum(flag) - flag, int(flag.sum()), offsets, max_voxels)


# ------------------------------------------------------------------------------------------------ sites
def _unique_rows(c):
    """np.unique(c, axis=0) of non-negative (n, 4) rows, through one linear key per row (much faster)"""
    c = np.asarray(c).astype(np.int64)
    m = c.max(0) + 1
    key = ((c[:, 0] * m[1] + c[:, 1]) * m[2] + c[:, 2]) * m[3] + c[:, 3]
    _, first = np.unique(key, return_index=True)
    return c[first]


def blob_sites(rng, B, shape, n, centres=400, spread=(2, 12, 12)):
    """clustered occupancy, so that summary words hold several blocks and blocks several cells; unique rows in random order"""
    c0 = np.stack([rng.integers(0, B, centres), rng.integers(0, shape[0], centres), rng.integers(0, shape[1], centres),
                   rng.integers(0, shape[2], centres)], 1)
    pick = c0[rng.integers(0, centres, 3 * n)]
    c = pick + np.round(rng.standard_normal((3 * n, 4)) * np.array([0, *spread])).astype(np.int64)
    ok = (c[:, 1] >= 0) & (c[:, 1] < shape[0]) & (c[:, 2] >= 0) & (c[:, 2] < shape[1]) & (c[:, 3] >= 0) & (c[:, 3] < shape[2])
    c = _unique_rows(c[ok])
    return c[rng.permutation(c.shape[0])][:n]


def edge_sites(rng, B, shape):
    """deliberate populations: the eight corners of scene 0 and of the last scene (2 x 2 x 2 cells each), sparse sheets on the six
    faces, a band straddling every multiple of 4 and 32 in y and x near one patch corner, and the last (for 180: partly filled)
    patch"""
    D, H, W = shape
    out = []
    for b in sorted({0, B - 1}):
        for z0 in (0, D - 2):
            for y0 in (0, H - 2):
                for x0 in (0, W - 2):
                    zz, yy, xx = np.meshgrid(np.arange(max(z0, 0), min(z0 + 2, D)), np.arange(y0, y0 + 2), np.arange(x0, x0 + 2), indexing="ij")
                    out.append(np.stack([np.full(zz.size, b), zz.ravel(), yy.ravel(), xx.ravel()], 1))
        m = 300
        for axis, size in ((1, D), (2, H), (3, W)):
            for v in (0, size - 1):
                c = np.stack([np.full(m, b), rng.integers(0, D, m), rng.integers(0, H, m), rng.integers(0, W, m)], 1)
                c[:, axis] = v
                out.append(c)
        # a band over the patch corner at (32 p, 32 q): every y and x of [32 p - 9, 32 p + 9) with all z of the lowest two blocks
        py, qx = 32 * min(2, (H - 10) // 32), 32 * min(3, (W - 10) // 32)
        if py >= 32 and qx >= 32:
            zz, yy, xx = np.meshgrid(np.arange(min(D, 6)), np.arange(py - 9, py + 9), np.arange(qx - 9, qx + 9), indexing="ij")
            keep = rng.random(zz.size) < 0.5
            out.append(np.stack([np.full(zz.size, b), zz.ravel(), yy.ravel(), xx.ravel()], 1)[keep])
        # the last patch of the plane
        y0, x0 = 32 * ((H - 1) // 32), 32 * ((W - 1) // 32)
        m = 400
        out.append(np.stack([np.full(m, b), rng.integers(0, D, m), rng.integers(y0, H, m), rng.integers(x0, W, m)], 1))
    return np.concatenate(out).astype(np.int64)


def boundary_sites(rng, B, shape, every_chunk=False, per=6):
    """cells in the last blocks before and the first blocks behind boundaries of a summary word, a unit, a group and a chunk of
    the prefix, picked by BLOCK ID (block_origin), so that the counts change exactly there; every_chunk: both ends of every chunk"""
    g = dims(B, shape)
    w = wpw(g["nsum"])
    sizes = [64, 64 * w, 64 * w * 64, 64 * w * 1024]
    blks = []
    for sz in sizes:
        nb = g["nblk"] // sz
        ms = np.arange(1, nb + 1) if (every_chunk and sz == sizes[-1]) else np.unique(rng.integers(1, max(nb, 1) + 1, per))
        for m in ms:
            blks.extend([m * sz - 2, m * sz - 1, m * sz, m * sz + 1])
    blks.extend([0, 1, g["nblk"] - 2, g["nblk"] - 1])
    blks = np.unique(np.array([v for v in blks if 0 <= v < g["nblk"]], np.int64))
    org, ok = block_origin(blks, B, shape)
    org = org[ok]
    out = []
    for _ in range(3):     # up to three cells per block
        c = org + np.concatenate([np.zeros((org.shape[0], 1), np.int64), rng.integers(0, 4, (org.shape[0], 3))], 1)
        out.append(c)
    c = np.concatenate(out)
    return c[(c[:, 1] < g["D"]) & (c[:, 2] < g["H"]) & (c[:, 3] < g["W"])]


def unique_rows(rng, parts, n=None):
    """the union of coordinate lists as unique rows in random order (int32), at most n of the FIRST part's rows dropped to fit"""
    c = _unique_rows(np.concatenate(parts))
    c = c[rng.permutation(c.shape[0])]
    return np.ascontiguousarray(c[:n] if n else c).astype(np.int32)


# ------------------------------------------------------------------------------------------------ comparators (no allowance)
class Mismatch(AssertionError):
    pass


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _take(a, ids):
    """a[ids] of a numpy array or of a torch tensor on any device, as numpy"""
    if hasattr(a, "detach"):
        import torch
        return a[torch.from_numpy(np.ascontiguousarray(ids)).to(a.device)].cpu().numpy()
    return np.asarray(a)[ids]


def _nnz(a):
    return int(a.count_nonzero()) if hasattr(a, "detach") else int(np.count_nonzero(a))


def _first_diff(got, want):
    d = np.nonzero(np.asarray(got != want).reshape(got.shape[0], -1).any(1))[0] if got.ndim else np.array([0])
    return f"{d.shape[0]} differ, first at {d[:6].tolist()}: got {got[d[:3]].tolist()}, want {want[d[:3]].tolist()}"


def equal(what, got, want):
    """array_equal of two arrays of one shape, or Mismatch naming the first rows that differ"""
    got, want = _np(got), _np(want)
    if got.shape != tuple(want.shape):
        raise Mismatch(f"{what}: shape {got.shape}, want {want.shape}")
    if not np.array_equal(got, want):
        raise Mismatch(f"{what}: {_first_diff(got, np.asarray(want).astype(got.dtype))}")


def gather_words(W, bits, base, summary, total):
    """what compare_words looks at, taken from the arrays as the device holds them (bits (nblk,), base (nblk,), summary (nsum,):
    any integer dtype of the right width, torch on any device or numpy): the words on the reference's occupied blocks and
    non-zero summary words, and the NUMBER of non-zero words (nothing may be set anywhere else)"""
    return dict(total=int(total), nnz_bits=_nnz(bits), nnz_summary=_nnz(summary),
                bits=_take(bits, W.blocks).astype(np.int64).view(np.uint64), summary=_take(summary, W.sum_ids).astype(np.int64).view(np.uint64),
                base=_take(base, W.blocks).astype(np.int64) & 0xFFFFFFFF)


def words_as_gathered(W):
    """a correct result in gather_words' form"""
    return dict(total=W.total, nnz_bits=W.blocks.shape[0], nnz_summary=W.sum_ids.shape[0], bits=W.bits.copy(), summary=W.sum_words.copy(),
                base=W.base.copy())


def compare_words(what, W, got):
    """got: gather_words(...).  The total, every occupied block's occupancy word and base, every summary word, nothing else set."""
    if got["total"] != W.total:
        raise Mismatch(f"{what}: total {got['total']}, want {W.total}")
    if got["nnz_bits"] != W.blocks.shape[0]:
        raise Mismatch(f"{what}: {got['nnz_bits']} occupied blocks, want {W.blocks.shape[0]}")
    if got["nnz_summary"] != W.sum_ids.shape[0]:
        raise Mismatch(f"{what}: {got['nnz_summary']} non-zero summary words, want {W.sum_ids.shape[0]}")
    equal(f"{what}: bits on occupied blocks", got["bits"], W.bits)
    equal(f"{what}: summary words", got["summary"], W.sum_words)
    equal(f"{what}: base on occupied blocks", got["base"], W.base)


def compare_table(what, got, want, n, prefill=None):
    """got (K, cap) against want (K, n) on every row below n; with prefill, the columns from n on must still hold it"""
    got = _np(got)
    equal(what, got[:, :n].astype(np.int64), want)
    if prefill is not None and not (got[:, n:] == prefill).all():
        raise Mismatch(f"{what}: written beyond row {n}")


def compare_rows(what, got, want, n, prefill=None):
    """got (cap, ...) against want (n, ...) row by row IN ORDER; with prefill, rows from n on must still hold it"""
    got = _np(got)
    equal(what, got[:n], _np(want))
    if prefill is not None:
        rest = got[n:]
        if not ((rest != rest) if prefill != prefill else (rest == prefill)).all():
            raise Mismatch(f"{what}: written beyond row {n}")
