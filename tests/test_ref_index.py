"""tests/ref_index.py, the coordinate-only reference of the at-scale index tests (tests/test_gpu_index_at_scale.py), checked on the
CPU: against the C oracle's rulebooks and voxeliser and against ref64's dense lookup on small random shapes; its rank order and
prefix against brute force and a hand-worked grid; and against PLANTED DEFECTS — what a subtly wrong index kernel would leave
behind, applied to a correct result — every one of which the comparators of ref_index must reject."""
import numpy as np
import pytest

import ref64 as R64
import ref_index as R

# (k, s, p) of the backbone: the SubM 3x3x3 layers and its four strided geometries
STRIDED = [(3, 2, 1), (3, 2, (0, 1, 1)), ((3, 1, 1), (2, 1, 1), 0), (2, 2, 0)]
SHAPES = [(2, [2, 23, 37]), (3, [5, 45, 70]), (2, [41, 37, 50])]      # D in {2, 5, 41}; H, W no multiples of 4 or of 32


def _random_sites(rng, B, shape, n):
    cells = B * shape[0] * shape[1] * shape[2]
    lin = rng.choice(cells, size=min(n, cells // 2), replace=False)
    b, rem = np.divmod(lin, shape[0] * shape[1] * shape[2])
    z, rem = np.divmod(rem, shape[1] * shape[2])
    y, x = np.divmod(rem, shape[2])
    return np.stack([b, z, y, x], 1).astype(np.int32)


def _oracle_pairs(pin, pout, pn):
    s = set()
    for k in range(pin.shape[0]):
        s |= set(zip([k] * int(pn[k]), pin[k, :pn[k]].tolist(), pout[k, :pn[k]].tolist()))
    return s


# ------------------------------------------------------------------------------------------------ against the oracle and ref64
@pytest.mark.parametrize("B,shape", SHAPES)
def test_subm_table_equals_the_dense_lookup_and_the_oracle(oracle, rng, B, shape):
    idx = _random_sites(rng, B, shape, 3000)
    for ksize in (3, (3, 1, 1), 1):
        nbr = R.neighbours_subm(idx, B, shape, ksize)
        assert np.array_equal(nbr, R64.neighbours_subm(idx, B, shape, ksize))
        assert R64.pairs_of(nbr) == _oracle_pairs(*oracle.rulebook_subm(idx, shape, ksize))
    assert np.array_equal(R.row_masks(R.neighbours_subm(idx, B, shape, 3)) >> 13 & 1, np.ones(idx.shape[0], np.int64))


# (a kernel of depth 3 without padding in z leaves no output plane on the D = 2 grid: those two pairs do not exist)
STRIDED_CASES = [(B, shape, *g) for B, shape in SHAPES for g in STRIDED + [(3, 1, 1)] if min(R.out_shape_of(shape, *g)) >= 1]
assert len(STRIDED_CASES) == 13


@pytest.mark.parametrize("B,shape,k,s,p", STRIDED_CASES)
def test_strided_table_equals_the_dense_lookup_and_the_oracle(oracle, rng, B, shape, k, s, p):
    idx = _random_sites(rng, B, shape, 2500)
    out, osh, nbr = R.neighbours_strided(idx, B, shape, k, s, p)
    # the sites in RANK order of the output grid: ascending (block, bit), each once
    key = R.rank_key(out, B, osh)
    assert (np.diff(key) > 0).all()
    d_out, d_osh, d_nbr = R64.neighbours_strided(idx, B, shape, k, s, p)        # (sorted by coordinate key)
    assert osh == d_osh
    m = R64.match_rows(d_out, out, osh)                                        # reference row -> dense row
    assert np.array_equal(d_out[m], out) and np.array_equal(d_nbr[:, m], nbr)
    o_idx, o_shape, pin, pout, pn = oracle.rulebook_strided(idx, shape, k, s, p)
    assert o_shape == osh
    mo = R64.match_rows(out, o_idx, osh)                                       # oracle row -> reference row
    assert R64.pairs_of(nbr) == {(kk, i, int(mo[o])) for kk, i, o in _oracle_pairs(pin, pout, pn)}


def test_first_come_order_equals_the_oracle_voxeliser(oracle, rng):
    vs, rg = [0.25, 0.25, 0.5], [-2.5, -2.5, -1.0, 2.5, 2.5, 1.0]
    grid = [20, 20, 4]
    scenes = []
    for s in range(5):
        p = rng.uniform(-3, 3, size=(0 if s == 2 else 700 + 31 * s, 5)).astype(np.float32)
        p[:, 2] = rng.uniform(-1.2, 1.2, size=p.shape[0])
        scenes.append(p)
    for max_voxels in (10000, 150):
        keys, want = [], []
        for b, p in enumerate(scenes):
            q = np.floor((p[:, :3] - np.float32(rg[:3])) / np.float32(vs))
            ok = ((q >= 0) & (q < np.array(grid))).all(1)
            c = q.astype(np.int64)
            keys.append(np.where(ok, ((b * grid[2] + c[:, 2]) * grid[1] + c[:, 1]) * grid[0] + c[:, 0], -1))
            _, oc, _ = oracle.voxelize(p, vs, rg, 4, max_voxels)
            want.append(((b * grid[2] + oc[:, 0].astype(np.int64)) * grid[1] + oc[:, 1]) * grid[0] + oc[:, 2])
        keys, want = np.concatenate(keys), np.concatenate(want)
        off = np.concatenate([[0], np.cumsum([p.shape[0] for p in scenes])])
        row, out_base, count = R.first_come(keys, off, max_voxels)
        got = np.full(int(count.sum()), -7, np.int64)
        got[row[row >= 0]] = keys[row >= 0]
        assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ rank order and prefix
def test_hand_worked_grid():
    """B = 2, [5, 40, 70]: bd = 2, bh = 10, bw = 18 -> th = 2, tw = 3 patches, 2 * 2 * 3 * 64 * 2 = 1 536 blocks, 24 summary words."""
    B, shape = 2, [5, 40, 70]
    g = R.dims(B, shape)
    assert (g["bd"], g["bh"], g["bw"], g["th"], g["tw"], g["nblk"], g["nsum"]) == (2, 10, 18, 2, 3, 1536, 24)
    idx = np.array([[0, 0, 0, 0],      # patch (0,0) col 0 bz 0                                          -> block 0, bit 0
                    [0, 4, 1, 2],      # same column, bz 1; bit 0*16 + 1*4 + 2                            -> block 1, bit 6
                    [0, 3, 3, 7],      # by 0, bx 1: col = m3(0) << 1 | m3(1) = 1; bit 3*16 + 3*4 + 3    -> block 2, bit 63
                    [0, 0, 4, 0],      # by 1, bx 0: col = m3(1) << 1 = 2                                 -> block 4, bit 0
                    [0, 0, 12, 20],    # by 3, bx 5: m3(3) = 0b101 = 5, m3(5) = 0b10001 = 17: col 10 | 17 = 27 -> block 54
                    [0, 0, 31, 31],    # by 7, bx 7: col 63; bit 0 + 3*4 + 3                              -> block 126, bit 15
                    [0, 1, 0, 32],     # patch (0,1): (0*3 + 1) * 64 = 64 columns before                  -> block 128, bit 16
                    [0, 0, 32, 0],     # patch (1,0): (1*3 + 0) * 64 columns                              -> block 384
                    [1, 0, 0, 0],      # scene 1: 2 * 3 * 64 columns                                      -> block 768
                    [1, 4, 39, 69]])   # patch (1,2), by 9 & 7 = 1, bx 17 & 7 = 1: col 3; ((6 + 5) * 64 + 3) * 2 + 1 = 1415; bit 0 + 3*4 + 1
    blk, bit = R.block_and_bit(idx, B, shape)
    assert blk.tolist() == [0, 1, 2, 4, 54, 126, 128, 384, 768, 1415]
    assert bit.tolist() == [0, 6, 63, 0, 0, 15, 16, 0, 0, 13]
    org, ok = R.block_origin(blk, B, shape)
    assert ok.all() and np.array_equal(org, idx & ~np.array([0, 3, 3, 3]))
    _, ok = R.block_origin(np.array([(5 * 64 + 63) * 2]), B, shape)     # patch (1,2) column 63: y 60, x 92 — beyond the grid
    assert not ok.any()
    rows = idx[[4, 9, 0, 2, 1, 7, 8, 3, 6, 5]]                          # any row order
    more = np.array([[0, 1, 1, 1], [0, 0, 0, 1], [1, 4, 39, 68]])       # block 0 bits 21 and 1; block 1415 bit 12
    rows = np.concatenate([rows, more])
    W = R.grid_words(rows, B, shape)
    assert W.blocks.tolist() == [0, 1, 2, 4, 54, 126, 128, 384, 768, 1415]
    assert W.bits.tolist() == [(1 << 0) | (1 << 1) | (1 << 21), 1 << 6, 1 << 63, 1, 1, 1 << 15, 1 << 16, 1, 1, (1 << 12) | (1 << 13)]
    assert W.base.tolist() == [0, 3, 4, 5, 6, 7, 8, 9, 10, 11] and W.total == 13
    assert W.sum_ids.tolist() == [0, 1, 2, 6, 12, 22]
    assert W.sum_words.tolist() == [(1 << 0) | (1 << 1) | (1 << 2) | (1 << 4) | (1 << 54), 1 << 62, 1, 1, 1, 1 << 7]
    # rank order: (block, bit) ascending -> rows (0,0,0,0) (0,0,0,1) (0,1,1,1) | block 1 | ...
    assert rows[R.rank_order(rows, B, shape)].tolist() == [[0, 0, 0, 0], [0, 0, 0, 1], [0, 1, 1, 1], [0, 4, 1, 2], [0, 3, 3, 7], [0, 0, 4, 0],
                                                            [0, 0, 12, 20], [0, 0, 31, 31], [0, 1, 0, 32], [0, 0, 32, 0], [1, 0, 0, 0],
                                                            [1, 4, 39, 68], [1, 4, 39, 69]]


@pytest.mark.parametrize("B,shape", SHAPES + [(2, [11, 180, 180])])
def test_rank_order_is_a_monotone_bijection_and_base_a_brute_force_count(rng, B, shape):
    idx = _random_sites(rng, B, shape, 4000)
    blk, bit = R.block_and_bit(idx, B, shape)
    g = R.dims(B, shape)
    assert blk.min() >= 0 and blk.max() < g["nblk"]
    org, ok = R.block_origin(blk, B, shape)
    assert ok.all() and np.array_equal(org, idx & ~np.array([0, 3, 3, 3]))
    perm, rank = R.rank_order(idx, B, shape), R.rank_of(idx, B, shape)
    assert np.array_equal(np.sort(perm), np.arange(idx.shape[0])) and np.array_equal(perm[rank], np.arange(idx.shape[0]))
    pairs = np.stack([blk[perm], bit[perm]], 1)
    assert (np.diff(pairs[:, 0] * 64 + pairs[:, 1]) > 0).all()
    W = R.grid_words(idx, B, shape)
    # brute force: cells in blocks before mine, one block at a time
    for j in rng.integers(0, W.blocks.shape[0], 200):
        assert W.base[j] == int((blk < W.blocks[j]).sum())
        assert R.popcount(W.bits[j:j + 1])[0] == int((blk == W.blocks[j]).sum())
    below = R.popcount(W.bits[np.searchsorted(W.blocks, blk)] & ((np.uint64(1) << bit.astype(np.uint64)) - np.uint64(1)))
    assert np.array_equal(W.base[np.searchsorted(W.blocks, blk)] + below, rank)       # rank = base + popcount below, the header's formula
    dense = np.zeros(g["nsum"] * 64, bool)
    dense[blk] = True
    want = np.packbits(dense.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).ravel()
    assert np.array_equal(np.nonzero(want)[0], W.sum_ids) and np.array_equal(want[W.sum_ids], W.sum_words)


def test_prefix_split_restated():
    assert [R.wpw(n) for n in (1, 32767, 32768, 262143, 262144, 1 << 22)] == [1, 1, 8, 8, 16, 16]
    prod = [41, 1440, 1440]
    table = {1: (22275, 1, 22275, 22), 2: (44550, 8, 5569, 6), 11: (245025, 8, 30629, 30), 12: (267300, 16, 16707, 17),
             48: (1069200, 16, 66825, 66), 128: (2851200, 16, 178200, 175)}
    for B, (nsum, w, u, c) in table.items():
        n = R.dims(B, prod)["nsum"]
        assert (n, R.wpw(n), R.units(n), R.chunks(n)) == (nsum, w, u, c)
    assert R.dims(128, [5, 180, 180])["nsum"] == 9216 and R.dims(128, [2, 180, 180])["nsum"] == 4608
    assert R.dims(128, [21, 720, 720])["nsum"] // 16 // 1024 + 1 == 25      # the benchmark's stage-2 grid: 25 chunks
    assert R.counter_words(22275) == 22275 + 349 + 22


def test_workgroup_table_load():
    blk = np.arange(600) // 2
    nb, nu = R.workgroup_table_load(blk, blk // 64)
    assert nb.tolist() == [128, 128, 44] and nu.tolist() == [2, 2, 1]
    two = np.stack([blk, np.where(blk % 2 == 0, blk + 1000, -1)], 1)
    nb, _ = R.workgroup_table_load(two, two // 64)
    assert nb.tolist() == [192, 192, 66]


# ------------------------------------------------------------------------------------------------ planted defects
@pytest.fixture(scope="module")
def big():
    """the 48-scene lidar grid (66 chunks of the prefix), sparsely filled with rows in every chunk: the reference is sparse"""
    rng = np.random.default_rng(7)
    B, shape = 48, [41, 1440, 1440]
    idx = R.unique_rows(rng, [R.blob_sites(rng, B, shape, 30000), R.boundary_sites(rng, B, shape, every_chunk=True)])
    g = R.dims(B, shape)
    W = R.grid_words(idx, B, shape)
    assert R.chunks(g["nsum"]) == 66 and np.unique(R.unit_of(W.blocks, g["nsum"]) >> 10).shape[0] == 66
    return idx, B, shape, g, W


def _rejected(fn, *a):
    with pytest.raises(R.Mismatch):
        fn(*a)


def test_planted_defects_in_the_grid_words(big):
    idx, B, shape, g, W = big
    good = R.words_as_gathered(W)
    R.compare_words("correct", W, good)
    unit = R.unit_of(W.blocks, g["nsum"])
    cnt = R.popcount(W.bits)

    def plant(**kw):
        d = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in good.items()}
        d.update(kw)
        return d
    # one mark missing: a bit of one block gone, every later base and the total one short
    j = W.blocks.shape[0] // 3
    bits = W.bits.copy()
    bits[j] &= bits[j] - np.uint64(1)
    base = W.base - (np.arange(W.base.shape[0]) > j)
    _rejected(R.compare_words, "mark missing", W, plant(bits=bits, base=base, total=W.total - 1,
                                                         nnz_bits=good["nnz_bits"] - int(bits[j] == 0)))
    _rejected(R.compare_words, "mark missing, total kept", W, plant(bits=bits))
    # one cell counted twice by the marks: every base behind its unit one up, and the total
    _rejected(R.compare_words, "counted twice", W, plant(base=W.base + (unit > unit[j]), total=W.total + 1))
    _rejected(R.compare_words, "counted twice, total kept", W, plant(base=W.base + (unit > unit[j])))
    # the second round of the lane-strided chunk loop lost: base short by the count of one chunk from chunk 64 on
    lost = int(cnt[(unit >> 10) == 63].sum())
    assert lost > 0 and ((unit >> 10) >= 64).any()
    _rejected(R.compare_words, "chunk 64 on", W, plant(base=W.base - lost * ((unit >> 10) >= 64)))
    # a group total missing: base short by one group's count from a group boundary on, inside one chunk
    grp = (unit >> 6)[j]
    lostg = int(cnt[(unit >> 6) == grp].sum())
    sel = ((unit >> 6) > grp) & ((unit >> 10) == (grp >> 4))
    assert lostg > 0 and sel.any()
    _rejected(R.compare_words, "group", W, plant(base=W.base - lostg * sel))
    # a summary bit missing / a stray word set somewhere else
    summ = W.sum_words.copy()
    summ[5] &= summ[5] - np.uint64(1)
    _rejected(R.compare_words, "summary bit", W, plant(summary=summ))
    _rejected(R.compare_words, "stray word", W, plant(nnz_bits=good["nnz_bits"] + 1))


def _planted_sites(rng):
    B, shape = 2, [9, 70, 45]
    seeds = np.array([[0, 3, 10, 44], [0, 3, 11, 0],      # x = W - 1 and the first cell of the next line
                      [1, 4, 31, 20], [1, 4, 32, 20],      # neighbours across the patch border y = 32
                      [1, 2, 40, 31], [1, 2, 40, 32]])     # ... and x = 32
    idx = R.unique_rows(rng, [_random_sites(rng, B, shape, 5000).astype(np.int64), seeds])
    return idx, B, shape, seeds


def test_planted_defects_in_tables_ranks_and_masks(rng):
    idx, B, shape, seeds = _planted_sites(rng)
    n = idx.shape[0]
    lut = R._Lookup(idx.astype(np.int64), shape)
    row = lambda c: int(lut.find(*[np.array([v]) for v in c])[0])
    nbr = R.neighbours_subm(idx, B, shape, 3)
    cap = n + 5
    table = np.full((27, cap), -2, np.int64)
    table[:, :n] = nbr
    R.compare_table("correct", table, nbr, n, prefill=-2)
    # written beyond n
    t = table.copy()
    t[3, n] = 0
    _rejected(R.compare_table, "beyond n", t, nbr, n, -2)
    # the wrapped-around cell: (y, W - 1) has no +x neighbour, the lookup without the bound test finds (y + 1, 0)
    a, b = row(seeds[0]), row(seeds[1])
    assert nbr[14, a] == -1
    t = table.copy()
    t[14, a] = b
    _rejected(R.compare_table, "wrap", t, nbr, n, -2)
    # a neighbour across a patch border reported absent (y then x)
    for lo, hi, k in ((seeds[2], seeds[3], 16), (seeds[4], seeds[5], 14)):
        a, b = row(lo), row(hi)
        assert nbr[k, a] == b and nbr[26 - k, b] == a
        t = table.copy()
        t[k, a] = -1
        _rejected(R.compare_table, "patch border", t, nbr, n, -2)
    # rows in another order with a permutation: perm not applied to one neighbour (the rank stands there instead of the row)
    perm, rank = R.rank_order(idx, B, shape), R.rank_of(idx, B, shape)
    k, o = np.nonzero(nbr >= 0)
    pick = np.nonzero(rank[nbr[k, o]] != nbr[k, o])[0][17]
    t = table.copy()
    t[k[pick], o[pick]] = rank[nbr[k[pick], o[pick]]]
    _rejected(R.compare_table, "perm not applied", t, nbr, n, -2)
    # two ranks swapped: in perm, and in the output rows of a strided layer (equal as SETS, which is why sets are not enough)
    R.compare_rows("correct perm", perm, perm, n)
    p2 = perm.copy()
    p2[[100, 101]] = p2[[101, 100]]
    _rejected(R.compare_rows, "ranks swapped", p2, perm, n)
    out, osh, snbr = R.neighbours_strided(idx, B, shape, 3, 2, 1)
    o2 = np.concatenate([out, np.full((3, 4), -2, np.int32)])
    R.compare_rows("correct sites", o2, out, out.shape[0], prefill=-2)
    o2[[40, 41]] = o2[[41, 40]]
    assert {tuple(r) for r in o2[:out.shape[0]].tolist()} == {tuple(r) for r in out.tolist()}
    _rejected(R.compare_rows, "sites swapped", o2, out, out.shape[0], -2)
    # one rowmask bit wrong
    masks = R.row_masks(nbr)
    assert np.array_equal(masks, np.array([sum(1 << kk for kk in range(27) if nbr[kk, o] >= 0) for o in range(0, n)]))
    R.compare_rows("correct masks", masks, masks, n)
    m2 = masks.copy()
    m2[n // 2] ^= 1 << 22
    _rejected(R.compare_rows, "rowmask bit", m2, masks, n)


def test_planted_defect_second_grid_stride_round_left_at_the_prefill(rng):
    n = R.GRID_STRIDE_ROWS + 1000
    want = rng.integers(-1, n, (3, n))
    got = np.full((3, n + 37), -2, np.int64)
    got[:, :n] = want
    R.compare_table("correct", got, want, n, prefill=-2)
    got[:, R.GRID_STRIDE_ROWS:n] = -2
    _rejected(R.compare_table, "second round", got, want, n, -2)


def _emit(keys, row, n_rows):
    out = np.full(n_rows, -7, np.int64)
    ok = (row >= 0) & (row < n_rows)
    out[row[ok]] = keys[ok]
    return out


def test_planted_defect_scene_64_starts_off_by_the_last_count_of_scene_63(rng):
    B, per, cells = 66, 300, 500
    keys = np.concatenate([b * cells + rng.integers(0, cells, per) for b in range(B)])
    off = np.arange(B + 1) * per
    flag = R.first_flags(keys)
    fc = np.cumsum(flag) - flag
    row, out_base, count = R.rows_from_scan(flag, fc, int(flag.sum()), off, 150)
    assert (count == 150).all()
    good = _emit(keys, row, int(count.sum()))
    R.compare_rows("correct", good, good, good.shape[0])
    # the running prefix not carried across the 64-scene round: the scenes of the second round start at 0 + their own prefix
    scene = np.repeat(np.arange(B), per)
    bad_row = np.where((row >= 0) & (scene >= 64), row - count[63], row)
    _rejected(R.compare_rows, "scene round", _emit(keys, bad_row, good.shape[0]), good, good.shape[0])


def test_planted_defect_first_come_ranks_short_by_one_tile_sum_from_point_1048576_on(rng):
    n, cells = 257 * R.SCAN_TILE + 1, 4000
    split = 256 * R.SCAN_TILE - 600       # scene 1 opens shortly before the 257th tile: its first points straddle the carry
    keys = np.concatenate([rng.integers(0, cells, split), cells + rng.integers(0, cells, n - split)])
    off = np.array([0, split, n])
    flag = R.first_flags(keys)
    assert flag[256 * R.SCAN_TILE:].sum() > 100
    fc = np.cumsum(flag) - flag
    total = int(flag.sum())
    row, _, count = R.rows_from_scan(flag, fc, total, off, 100000)
    good = _emit(keys, row, total)
    assert (good >= 0).all()
    tile_sum = int(flag[255 * R.SCAN_TILE:256 * R.SCAN_TILE].sum())
    assert tile_sum > 0
    fc_bad = fc - tile_sum * (np.arange(n) >= 256 * R.SCAN_TILE)
    row_bad, _, _ = R.rows_from_scan(flag, fc_bad, total - tile_sum, off, 100000)
    _rejected(R.compare_rows, "scan carry", _emit(keys, row_bad, total), good, total)
