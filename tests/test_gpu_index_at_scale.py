"""The index machinery under every convolution — the voxeliser (csrc/voxelize.hip), the device scans and the rank-grid prefix
(csrc/scan.hip, csrc/rankgrid.h), the rulebook builders (csrc/rulebook.hip) — against the coordinate-only numpy reference of
tests/ref_index.py AT THE SIZES THE BENCHMARK RUNS: every split of the prefix (1 / 8 / 16 summary words per wave), more than 64
chunks, the counted marks against the three-launch prefix, crowded LDS tables, more than 64 scenes, more than 256 scan tiles, a
second grid-stride round, and the production geometry (H, W no multiples of 32, D no multiple of 4).  Integer work: every
comparison is array_equal, every row below n and every occupied block is compared, and the output rows of the strided layers are
compared IN ORDER (scene, patch, Z-order column, block bottom to top, bit — rankgrid.h), not as sets.

THE GRIDS — the smallest at which each form exists.  The lidar grid [41, 1440, 1440] has bd = 11, bh = bw = 360 = 45 patches of
8 blocks: 45 * 45 * 64 * 11 = 1 425 600 blocks = 22 275 summary words per scene.  The prefix (fnp_rg_wpw) takes 1 word per wave
below 2^15 = 32 768 words, 8 from there, 16 from 2^18 = 262 144:

    G1    B = 1     22 275 words   wpw 1    22 275 units   22 chunks of 1 024 units
    G8    B = 2     44 550         wpw 8     5 569 units
    G16   B = 12   267 300         wpw 16   16 707 units   17 chunks      (B = 11: 245 025 < 2^18)
    G16c  B = 48 1 069 200         wpw 16   66 825 units   66 chunks > 64 (B = 47: 65 433 units = 64 chunks: the lane-strided sums
                                                                           over the chunk totals take a second round from 65)
    S4    B = 128  [5, 180, 180]: bd = 2, bh = 45 -> 6 patches (the last partly filled: y, x 160 .. 179), 128 * 36 * 64 * 2 / 64 = 9 216, wpw 1
    S5    B = 128  [2, 180, 180]: bd = 1                                                                                     4 608, wpw 1

Every case prints a FORM line (n, nsum, wpw, units, chunks) and asserts the dispatch condition it relies on."""

import numpy as np
import pytest
import torch

import ref_index as R
from findnpropagate_amd import lib as _l
from findnpropagate_amd import sparse as S
from findnpropagate_amd import synthetic as syn
from oracle import tile_rulebook as TR

pytestmark = pytest.mark.gpu

LIDAR = [41, 1440, 1440]
GRIDS = {   # name: (B, shape, nsum, wpw, chunks, rows asked of the blob generator)
    "G1": (1, LIDAR, 22275, 1, 22, 60000),
    "G8": (2, LIDAR, 44550, 8, 6, 120000),
    "G16": (12, LIDAR, 267300, 16, 17, 300000),
    "G16c": (48, LIDAR, 1069200, 16, 66, 150000),
    "S4": (128, [5, 180, 180], 9216, 1, 9, 100000),
    "S5": (128, [2, 180, 180], 4608, 1, 5, 60000),
    "G16big": (12, LIDAR, 267300, 16, 17, 600001),     # two grid-stride rounds of the row-parallel builders
}
for _name, (_B, _shape, _nsum, _w, _ch, _) in GRIDS.items():
    assert R.dims(_B, _shape)["nsum"] == _nsum and R.wpw(_nsum) == _w and R.chunks(_nsum) == _ch, _name
assert R.chunks(R.dims(47, LIDAR)["nsum"]) == 64 and R.wpw(R.dims(11, LIDAR)["nsum"]) == 8

GEOMS = [(3, 2, 1), (3, 2, (0, 1, 1)), ((3, 1, 1), (2, 1, 1), 0), (2, 2, 0)]      # the backbone's strided layers


# ------------------------------------------------------------------------------------------------ sites and references (cached per process)
_SITES, _REF = {}, {}


def sites(name):
    if name not in _SITES:
        B, shape, nsum, _, _, n = GRIDS[name]
        rng = np.random.default_rng(sorted(GRIDS).index(name) + 100)
        extra = [R.edge_sites(rng, B, shape), R.boundary_sites(rng, B, shape, every_chunk=(name == "G16c"))]
        m = sum(e.shape[0] for e in extra)
        blobs = R.blob_sites(rng, B, shape, n, centres=1200 if n > 400000 else 400)
        if name == "G16big":     # exactly n rows: blob rows make room for the deliberate ones
            idx = R.unique_rows(rng, [blobs[:n - m]] + extra)
            lin = lambda c: ((c[:, 0].astype(np.int64) * shape[0] + c[:, 1]) * shape[1] + c[:, 2]) * shape[2] + c[:, 3]
            more = blobs[n - m:]
            more = more[~np.isin(lin(more), lin(idx))][:n - idx.shape[0]]
            idx = np.ascontiguousarray(np.concatenate([idx, more.astype(np.int32)]))
            assert idx.shape[0] == n and np.unique(lin(idx)).shape[0] == n
        else:
            idx = R.unique_rows(rng, [blobs] + extra)
        _SITES[name] = idx
    return _SITES[name]


def ref(name):
    """idx (random row order), W (grid words), perm (rank -> row), rank (row -> rank)"""
    if name not in _REF:
        B, shape = GRIDS[name][:2]
        idx = sites(name)
        _REF[name] = dict(idx=idx, W=R.grid_words(idx, B, shape), perm=R.rank_order(idx, B, shape), rank=R.rank_of(idx, B, shape))
    return _REF[name]


def ref_subm(name, ksize=3):
    """(table of the rows in their random order, table of the rows in rank order)"""
    k = (name, "subm", str(ksize))
    if k not in _REF:
        B, shape = GRIDS[name][:2]
        r = ref(name)
        nbr = R.neighbours_subm(r["idx"], B, shape, ksize)
        sub = nbr[:, r["perm"]]
        _REF[k] = (nbr, np.where(sub >= 0, r["rank"][np.maximum(sub, 0)], -1))
    return _REF[k]


def ref_strided(name, geom):
    k = (name, "strided", str(geom))
    if k not in _REF:
        B, shape = GRIDS[name][:2]
        out, osh, nbr = R.neighbours_strided(ref(name)["idx"], B, shape, *geom)
        _REF[k] = (out, osh, nbr, R.grid_words(out, B, osh))
    return _REF[k]


def form(case, B, shape, n, **more):
    """the FORM line of a case; the summary word count comes from the library"""
    nsum = int(_l.load().fnp_rankgrid_num_summary(B, *shape))
    assert nsum == R.dims(B, shape)["nsum"]
    f = dict(n=int(n), nsum=nsum, wpw=R.wpw(nsum), units=R.units(nsum), chunks=R.chunks(nsum), **more)
    print(f"\nFORM {case} | B {B} shape {list(shape)} | " + " | ".join(f"{k} {v}" for k, v in f.items()))
    return f


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _padded(idx, cap, cuda):
    """(cap, 4) device rows: idx, then rows no kernel may read (they name cell 0 of scene 0: a read would show in the words)"""
    t = torch.zeros((cap, 4), dtype=torch.int32, device=cuda)
    t[:idx.shape[0]] = _dev(idx, cuda)
    return t


# ------------------------------------------------------------------------------------------------ entry points, outputs prefilled
def build(idx_dev, n_dev, B, shape, keep_order, grid=None):
    """fnp_rankgrid_build (always the three-launch prefix: its marking kernel does not count) -> (grid, total)"""
    L = _l.load()
    cap = idx_dev.shape[0]
    dev = idx_dev.device
    if grid is None:
        grid = S.alloc_grid(B, shape, dev, with_perm_cap=cap if keep_order else None)
    if keep_order:
        if grid.perm is None or grid.perm.numel() < cap:
            grid.perm = torch.empty((cap,), dtype=torch.int32, device=dev)
        grid.perm.fill_(-2)
    ws = torch.empty((int(L.fnp_rankgrid_workspace_bytes(B, *shape)) + 256,), dtype=torch.uint8, device=dev)
    _l.check(L.fnp_rankgrid_build(_l.ptr(idx_dev), _l.ptr(n_dev), cap, grid.c(with_perm=keep_order), _l.ptr(ws), ws.numel(), _l.stream()),
             "fnp_rankgrid_build")
    return grid, int(ws[:4].view(torch.int32).item())


class Strided:
    pass


def strided(idx_dev, n_dev, grid, geom, cap_out, out_grid=None, want_nbr=True, premarked=False, slack=64):
    """fnp_rulebook_strided[_premarked] with out_indices, out_n and nbr prefilled with -2 and `slack` words behind each"""
    L = _l.load()
    dev = idx_dev.device
    g, out_shape = S.make_geom(*geom, grid.shape)
    K = g.ksize[0] * g.ksize[1] * g.ksize[2]
    r = Strided()
    r.out_grid = out_grid if out_grid is not None else S.alloc_grid(grid.batch_size, out_shape, dev)
    r.out_shape, r.K, r.cap_out = out_shape, K, cap_out
    r.out_idx = torch.full((cap_out + slack, 4), -2, dtype=torch.int32, device=dev)
    r.out_n = torch.full((1,), -2, dtype=torch.int32, device=dev)
    flat = torch.full((K * cap_out + slack,), -2, dtype=torch.int32, device=dev) if want_nbr else None
    ws = torch.empty((int(L.fnp_rankgrid_workspace_bytes(grid.batch_size, *out_shape)),), dtype=torch.uint8, device=dev)
    fn = L.fnp_rulebook_strided_premarked if premarked else L.fnp_rulebook_strided
    _l.check(fn(_l.ptr(idx_dev), _l.ptr(n_dev), idx_dev.shape[0], g, grid.c(), r.out_grid.c(with_perm=False), _l.ptr(r.out_idx), _l.ptr(r.out_n),
                cap_out, _l.ptr(flat), _l.ptr(ws), ws.numel(), _l.stream()), "fnp_rulebook_strided")
    r.nbr = flat[:K * cap_out].view(K, cap_out) if want_nbr else None
    r.tail = flat[K * cap_out:] if want_nbr else None
    return r


class Subm:
    pass


def subm(idx_dev, n_dev, grid, ksize, kind="plain", mark_next=None):
    """the SubM rulebook entry points with the table (and row masks) prefilled with -2.  kind: plain | masked | tile32 | tile64 |
    lean32 | lean64; mark_next = (out_grid, geom) for the masked and lean kinds"""
    L = _l.load()
    dev = idx_dev.device
    cap = idx_dev.shape[0]
    g, _ = S.make_geom(ksize, 1, [k // 2 for k in R._triple(ksize)], grid.shape, grid.shape)
    r = Subm()
    r.K = g.ksize[0] * g.ksize[1] * g.ksize[2]
    r.nbr = torch.full((r.K, cap), -2, dtype=torch.int32, device=dev)
    mg = mgeom = None
    if mark_next is not None:
        mgeom, _ = S.make_geom(*mark_next[1], grid.shape)
        mg = mark_next[0].c(with_perm=False)
    a = (_l.ptr(idx_dev), _l.ptr(n_dev), cap, g, grid.c(), _l.ptr(r.nbr))
    if kind == "plain":
        rc = L.fnp_rulebook_subm(*a, _l.stream())
    elif kind == "masked":
        r.rowmask = torch.full((cap,), -2, dtype=torch.int32, device=dev)
        rc = L.fnp_rulebook_subm_masked(*a, _l.ptr(r.rowmask), mg, mgeom, _l.stream())
    else:
        r.channels = int(kind[-2:])
        r.tile = torch.zeros((int(L.fnp_tile_rulebook_bytes(cap, r.channels)),), dtype=torch.uint8, device=dev)
        if kind.startswith("lean"):
            r.esc = torch.zeros((1,), dtype=torch.int32, device=dev)
            rc = L.fnp_rulebook_subm_tiled_lean(*a, r.channels, _l.ptr(r.tile), mg, mgeom, _l.ptr(r.esc), _l.stream())
        else:
            rc = L.fnp_rulebook_subm_tiled(*a, r.channels, _l.ptr(r.tile), _l.stream())
    _l.check(rc, "fnp_rulebook_subm " + kind)
    return r


def clear(kind, jobs, monkeypatch):
    """kind: row (fnp_rankgrid_clear per grid) | rows (fnp_rankgrid_clear_multi) | summary (fnp_rankgrid_clear_summary)"""
    if kind == "row":
        for g, rows, n_dev in jobs:
            S.clear_grid(g, rows, n_dev)
        return
    monkeypatch.setattr(S, "CLEAR_BY_SUMMARY", kind == "summary")
    S.clear_grids(jobs)


# ------------------------------------------------------------------------------------------------ checks
def check_words(what, W, g, total):
    R.compare_words(what, W, R.gather_words(W, g.bits, g.base, g.summary, total))


def check_counters(what, W, g, counted):
    """the counter words: zero after an uncounted build; after a counted one the cells per unit, then per group of 64 units, then
    per chunk of 1 024 units, and zero behind them"""
    got = g.counters.cpu().numpy().astype(np.int64)
    nsum = g.summary.numel()
    want = np.zeros_like(got)
    if counted:
        u, cnt = R.unit_of(W.blocks, nsum), R.popcount(W.bits)
        nu, ng = R.units(nsum), R.groups(nsum)
        want[:nu] = np.bincount(u, weights=cnt, minlength=nu)
        want[nu:nu + ng] = np.bincount(u >> 6, weights=cnt, minlength=ng)
        want[nu + ng:nu + ng + R.chunks(nsum)] = np.bincount(u >> 10, weights=cnt, minlength=R.chunks(nsum))
    R.equal(f"{what}: counter words", got, want)


def assert_zero(what, g):
    nz = (int(g.bits.count_nonzero()), int(g.summary.count_nonzero()), int(g.counters.count_nonzero()))
    assert nz == (0, 0, 0), f"{what}: non-zero (bits, summary, counter) words left: {nz}"


def check_strided(what, r, out, osh, nbr, W_out, counted=None):
    m = out.shape[0]
    assert int(r.out_n.item()) == m, (what, int(r.out_n.item()), m)
    assert r.out_shape == osh
    lim = min(m, r.cap_out)
    R.compare_rows(f"{what}: output sites in rank order", r.out_idx, out[:lim], lim, prefill=-2)
    if r.nbr is not None:
        R.compare_table(f"{what}: table", r.nbr, nbr[:, :lim], lim, prefill=-2)
        assert bool((r.tail == -2).all()), f"{what}: written behind the table"
    check_words(f"{what}: output grid", W_out, r.out_grid, m)
    if counted is not None:
        check_counters(f"{what}: output grid", W_out, r.out_grid, counted)


# ------------------------------------------------------------------------------------------------ (a) grid words
def _grid_words_case(name, cuda, monkeypatch):
    B, shape, nsum, w, ch, _ = GRIDS[name]
    r = ref(name)
    idx, W, n = r["idx"], r["W"], r["idx"].shape[0]
    f = form(f"words {name}", B, shape, n)
    assert (f["nsum"], f["wpw"], f["chunks"]) == (nsum, w, ch)
    assert np.unique(R.unit_of(W.blocks, nsum) >> 10).shape[0] == ch, "every chunk of the prefix holds rows"
    idx_dev, n_dev = _dev(idx, cuda), S.device_scalar(n, cuda)
    grids = {}
    for keep in (True, False):
        for counters in (True, False):     # (the grid's counter words handed to the entry point or not: the prefix is the three-launch one)
            monkeypatch.setattr(S, "COUNTED_MARKS", counters)
            g, total = build(idx_dev, n_dev, B, shape, keep)
            what = f"{name} build keep_order={keep} counters={counters}"
            check_words(what, W, g, total)
            check_counters(what, W, g, False)
            if keep:
                R.compare_rows(f"{what}: perm", g.perm, r["perm"], n)
            grids[keep] = g
    # the COUNTED prefix: a 1x1x1 stride-1 layer marks its inputs' own cells in a second grid through the counting LDS tables, and
    # emits them in rank order: output row r is input row perm[r]
    geom = (1, 1, 0)
    for counted in (True, False):
        monkeypatch.setattr(S, "COUNTED_MARKS", counted)
        s = strided(idx_dev, n_dev, grids[True], geom, n + 37)
        check_strided(f"{name} 1x1x1 counted={counted}", s, idx[r["perm"]], list(shape), r["perm"][None, :], W, counted=counted)
        assert torch.equal(s.out_grid.bits, grids[True].bits) and torch.equal(s.out_grid.summary, grids[True].summary), "counted and uncounted builds give the same words"
        if counted:
            counted_grid, rows = s.out_grid, (s.out_idx, s.out_n)
    return grids, counted_grid, rows, idx_dev, n_dev


@pytest.mark.parametrize("name", ["G1", "G8", "G16", "S4", "S5"])
def test_grid_words(cuda, monkeypatch, name):
    grids, counted_grid, rows, idx_dev, n_dev = _grid_words_case(name, cuda, monkeypatch)
    # ... and the clears leave every word zero, the counters included
    monkeypatch.setattr(S, "COUNTED_MARKS", True)
    clear("row", [(grids[True], idx_dev, n_dev)], monkeypatch)
    assert_zero(f"{name} row clear", grids[True])
    clear("summary", [(grids[False], idx_dev, n_dev), (counted_grid, *rows)], monkeypatch)
    assert_zero(f"{name} summary clear", grids[False])
    assert_zero(f"{name} summary clear of the counted grid", counted_grid)


def test_grid_words_beyond_64_chunks(cuda, monkeypatch):
    """G16c: 66 chunks — the lane-strided sums over the chunk totals (cells before my unit; the grand total) run a second round"""
    assert GRIDS["G16c"][4] > 64
    grids, counted_grid, rows, idx_dev, n_dev = _grid_words_case("G16c", cuda, monkeypatch)
    monkeypatch.setattr(S, "COUNTED_MARKS", True)
    clear("summary", [(counted_grid, *rows)], monkeypatch)
    assert_zero("G16c summary clear", counted_grid)
    clear("rows", [(grids[True], idx_dev, n_dev), (grids[False], idx_dev, n_dev)], monkeypatch)
    assert_zero("G16c row clear", grids[True])
    assert_zero("G16c row clear", grids[False])


# ------------------------------------------------------------------------------------------------ (b) SubM tables
def _check_subm(what, s, want, n, kind):
    if kind in ("plain", "masked", "tile32", "tile64"):
        R.compare_table(f"{what}: table", s.nbr, want, n, prefill=-2)
    if kind == "masked":
        R.compare_rows(f"{what}: row masks", s.rowmask, R.row_masks(want).astype(np.int32), n, prefill=-2)
    if kind[:4] in ("tile", "lean"):
        got, esc = TR.decode(s.tile.cpu().numpy(), n, s.channels)
        escaped = got == -2
        R.equal(f"{what}: tile rulebook entries", np.where(escaped, want, got), want)
        if kind.startswith("lean"):     # the table holds what it promises: the rows of tiles with an escape entry
            tile = TR.GEOMETRY[s.channels][0]
            tiles = _tiles_with_escape(escaped, tile)
            assert np.array_equal(esc.astype(bool).any(1), tiles), f"{what}: escape flags name other tiles than the entries"
            rows = np.repeat(tiles, tile)[:n]
            R.equal(f"{what}: lean table on escape tiles", s.nbr[:, :n].cpu().numpy().astype(np.int64)[:, rows], want[:, rows])
            print(f"      {what}: {int(rows.sum())} of {n} rows in escape tiles")


def _tiles_with_escape(escaped, tile):
    n = escaped.shape[1]
    pad = np.zeros((escaped.shape[0], -(-n // tile) * tile), bool)
    pad[:, :n] = escaped
    return pad.reshape(escaped.shape[0], -1, tile).any(axis=(0, 2))


KINDS = ["plain", "masked", "tile32", "tile64", "lean32", "lean64"]


@pytest.mark.parametrize("order", ["rank", "random+perm"])
@pytest.mark.parametrize("name", ["G8", "G16", "S4"])
def test_subm_tables(cuda, name, order):
    B, shape, nsum, w, _, _ = GRIDS[name]
    r = ref(name)
    n = r["idx"].shape[0]
    f = form(f"subm {name} {order}", B, shape, n, rounds=-(-n // R.GRID_STRIDE_ROWS))
    assert f["wpw"] == w
    by_row, by_rank = ref_subm(name)
    idx, want = (r["idx"][r["perm"]], by_rank) if order == "rank" else (r["idx"], by_row)
    idx_dev, n_dev = _dev(idx, cuda), S.device_scalar(n, cuda)
    grid, _ = build(idx_dev, n_dev, B, shape, keep_order=(order != "rank"))
    for kind in KINDS:
        _check_subm(f"{name} {order} {kind}", subm(idx_dev, n_dev, grid, 3, kind), want, n, kind)
    if name == "G8":     # the generic kernel: one launch row per offset
        for ksize in ((3, 1, 1), 1):
            a, b = ref_subm(name, ksize)
            R.compare_table(f"{name} {order} k={ksize}", subm(idx_dev, n_dev, grid, ksize).nbr, b if order == "rank" else a, n, prefill=-2)


@pytest.mark.parametrize("slack", [37, 3])
def test_subm_tables_in_the_second_grid_stride_round(cuda, slack):
    """600 001 rows: the row-parallel builders (2 048 workgroups of 256 rows) run a second round, and nbr_flush writes at the
    offsets of that round — 4 bytes per lane for a table stride that is no multiple of 4, 16 bytes otherwise"""
    B, shape = GRIDS["G16big"][:2]
    r = ref("G16big")
    n = r["idx"].shape[0]
    cap = n + slack
    f = form(f"subm G16big cap n+{slack}", B, shape, n, cap=cap, rounds=-(-n // R.GRID_STRIDE_ROWS), scalar_flush=int(cap % 4 != 0))
    assert n == 600001 and f["rounds"] == 2 and f["wpw"] == 16 and (cap % 4 != 0) == (slack == 37)
    _, want = ref_subm("G16big")
    idx_dev, n_dev = _padded(r["idx"][r["perm"]], cap, cuda), S.device_scalar(n, cuda)
    grid, total = build(idx_dev, n_dev, B, shape, keep_order=False)
    check_words("G16big", r["W"], grid, total)
    assert bool((want[:, R.GRID_STRIDE_ROWS:] >= 0).any(1).all()), "every offset has entries in the second round"
    for kind in (["plain", "masked", "tile64"] if slack == 37 else ["plain", "masked", "lean32"]):
        _check_subm(f"G16big cap n+{slack} {kind}", subm(idx_dev, n_dev, grid, 3, kind), want, n, kind)


# ------------------------------------------------------------------------------------------------ (c) strided rulebooks
@pytest.mark.parametrize("geom", GEOMS, ids=["k3s2p1", "k3s2p011", "k311s211p0", "k2s2p0"])
@pytest.mark.parametrize("name", ["G8", "G16"])
def test_strided_rulebooks(cuda, monkeypatch, name, geom):
    B, shape, _, w, _, _ = GRIDS[name]
    r = ref(name)
    idx, n = r["idx"], r["idx"].shape[0]
    out, osh, nbr, W_out = ref_strided(name, geom)
    m = out.shape[0]
    f = form(f"strided {name} {geom}", B, shape, n)
    fo = form(f"strided {name} {geom} output grid", B, osh, m)
    assert f["wpw"] == w and all((R._triple(geom[0])[d] + R._triple(geom[1])[d] - 1) // R._triple(geom[1])[d] <= 2 for d in range(3)), "closed-form marks"
    if geom == (2, 2, 0):     # closed form: the output sites are the inputs' coordinates halved
        half = np.unique(np.concatenate([idx[:, :1], idx[:, 1:] // 2], 1)[(idx[:, 1:] // 2 < np.array(osh)).all(1)], axis=0)
        assert np.array_equal(half, np.unique(out, axis=0)) and half.shape[0] == m
    idx_dev, n_dev = _dev(idx, cuda), S.device_scalar(n, cuda)
    grid, _ = build(idx_dev, n_dev, B, shape, keep_order=True)     # (rows in random order: the marks visit them through perm)
    cap_out = m + 5
    first = None
    for counted in (True, False):
        monkeypatch.setattr(S, "COUNTED_MARKS", counted)
        s = strided(idx_dev, n_dev, grid, geom, cap_out)
        check_strided(f"{name} {geom} counted={counted}", s, out, osh, nbr, W_out, counted=counted)
        first = first or s
    monkeypatch.setattr(S, "COUNTED_MARKS", True)
    s = strided(idx_dev, n_dev, grid, geom, cap_out, want_nbr=False)
    check_strided(f"{name} {geom} want_nbr=False", s, out, osh, nbr, W_out, counted=True)
    assert torch.equal(s.out_idx, first.out_idx)
    # premarked: the SubM rulebook kernel of the input rows marks the output sites on the way (uncounted: three-launch prefix)
    by_row, _ = ref_subm(name)
    for kind in ("masked", "lean32", "lean64"):
        og = S.alloc_grid(B, osh, cuda)
        sm = subm(idx_dev, n_dev, grid, 3, kind, mark_next=(og, geom))
        _check_subm(f"{name} {geom} {kind} + marks", sm, by_row, n, kind)
        s = strided(idx_dev, n_dev, grid, geom, cap_out, out_grid=og, premarked=True)
        check_strided(f"{name} {geom} premarked by {kind}", s, out, osh, nbr, W_out, counted=False)
        assert torch.equal(s.out_idx, first.out_idx) and torch.equal(s.nbr, first.nbr) and torch.equal(s.out_n, first.out_n)
        assert torch.equal(og.bits, first.out_grid.bits) and torch.equal(og.summary, first.out_grid.summary)
    clear("rows", [(first.out_grid, first.out_idx, first.out_n), (grid, idx_dev, n_dev)], monkeypatch)
    assert_zero(f"{name} {geom} row clear of the output grid", first.out_grid)
    assert_zero(f"{name} {geom} row clear of the input grid", grid)


def test_strided_generic_marking_loop(cuda, monkeypatch):
    """(3, 1, 1): three outputs per input cell and axis — the marking loop over the kernel volume, never counted"""
    B, shape, geom = 2, [9, 40, 41], (3, 1, 1)
    rng = np.random.default_rng(5)
    idx = R.unique_rows(rng, [R.blob_sites(rng, B, shape, 3000, centres=12, spread=(2, 5, 5)), R.edge_sites(rng, B, shape)])
    n = idx.shape[0]
    form("strided generic marks", B, shape, n)
    assert (3 + 1 - 1) // 1 == 3
    out, osh, nbr = R.neighbours_strided(idx, B, shape, *geom)
    idx_dev, n_dev = _dev(idx, cuda), S.device_scalar(n, cuda)
    for keep in (True, False):
        rows = idx if keep else idx[R.rank_order(idx, B, shape)]
        want = nbr if keep else np.where(nbr >= 0, R.rank_of(idx, B, shape)[np.maximum(nbr, 0)], -1)
        rows_dev = _dev(rows, cuda)
        grid, _ = build(rows_dev, n_dev, B, shape, keep)
        s = strided(rows_dev, n_dev, grid, geom, out.shape[0] + 3)
        check_strided(f"generic marks keep_order={keep}", s, out, osh, want, R.grid_words(out, B, osh), counted=False)


def test_strided_second_grid_stride_round_in_and_out(cuda, monkeypatch):
    """more than 524 288 input rows AND output rows: strided_mark2_kernel (with its prefetch of the next round), the coordinate
    emission and strided_nbr_row_kernel all run a second round"""
    B, shape = GRIDS["G16big"][:2]
    geom = ((3, 1, 1), (2, 1, 1), 0)
    r = ref("G16big")
    idx, n = r["idx"], r["idx"].shape[0]
    out, osh, nbr, W_out = ref_strided("G16big", geom)
    m = out.shape[0]
    form("strided G16big", B, shape, n, out_rows=m, rounds_in=-(-n // R.GRID_STRIDE_ROWS), rounds_out=-(-m // R.GRID_STRIDE_ROWS))
    assert n > R.GRID_STRIDE_ROWS and m > R.GRID_STRIDE_ROWS
    idx_dev, n_dev = _dev(idx, cuda), S.device_scalar(n, cuda)
    grid, _ = build(idx_dev, n_dev, B, shape, keep_order=True)
    for counted in (True, False):
        monkeypatch.setattr(S, "COUNTED_MARKS", counted)
        s = strided(idx_dev, n_dev, grid, geom, m + 37)
        check_strided(f"G16big {geom} counted={counted}", s, out, osh, nbr, W_out, counted=counted)


def test_strided_output_capacity_below_the_true_count(cuda, monkeypatch):
    """cap_out < the number of output sites: out_n is the TRUE count, the rows below cap_out are right, nothing is written beyond,
    and the grid — which holds sites that have no row — still clears to zero through its summary level"""
    name, geom = "G8", (3, 2, 1)
    B, shape = GRIDS[name][:2]
    r = ref(name)
    idx, n = r["idx"], r["idx"].shape[0]
    out, osh, nbr, W_out = ref_strided(name, geom)
    m = out.shape[0]
    cap_out = (m * 2 // 3) | 1
    form("strided overflow", B, shape, n, out_rows=m, cap_out=cap_out)
    assert cap_out < m
    idx_dev, n_dev = _dev(idx, cuda), S.device_scalar(n, cuda)
    grid, _ = build(idx_dev, n_dev, B, shape, keep_order=True)
    s = strided(idx_dev, n_dev, grid, geom, cap_out)
    check_strided("overflow", s, out, osh, nbr, W_out, counted=True)
    clear("summary", [(s.out_grid, s.out_idx, s.out_n)], monkeypatch)
    assert_zero("overflow: summary clear", s.out_grid)
    # the cleared grid is as good as new: other inputs (half of the rows), counted prefix, word for word
    idx2 = np.ascontiguousarray(idx[:n // 2])
    out2, osh2, nbr2 = R.neighbours_strided(idx2, B, shape, *geom)
    i2_dev, n2_dev = _dev(idx2, cuda), S.device_scalar(idx2.shape[0], cuda)
    grid2, _ = build(i2_dev, n2_dev, B, shape, keep_order=True)
    s2 = strided(i2_dev, n2_dev, grid2, geom, out2.shape[0], out_grid=s.out_grid)
    check_strided("after the overflow", s2, out2, osh2, nbr2, R.grid_words(out2, B, osh2), counted=True)


# ------------------------------------------------------------------------------------------------ (d) crowded LDS tables
def test_crowded_mark_table(cuda, monkeypatch):
    """Isolated rank-ordered rows at (7, 7, 7) mod 16 of the lidar grid under k3 s2 p1: every row has 2 x 2 x 2 outputs, at cells
    3 | 4 mod 8 — across a block border on every axis — in 8 blocks no other row touches.  A workgroup's 256 rows put 2 048
    blocks into a mark table of 512 slots: most go straight to memory, the count with them."""
    B, shape, geom = 2, LIDAR, (3, 2, 1)
    yy, xx = np.meshgrid(np.arange(7, 1440, 16), np.arange(7, 1440, 16), indexing="ij")
    one = np.stack([np.zeros(yy.size, np.int64), np.full(yy.size, 7), yy.ravel(), xx.ravel()], 1)
    idx = np.concatenate([one, one + np.array([1, 16, 0, 0])]).astype(np.int32)
    idx = np.ascontiguousarray(idx[R.rank_order(idx, B, shape)])
    n = idx.shape[0]
    blocks = R.output_blocks(idx, B, shape, *geom)
    osh = R.out_shape_of(shape, *geom)
    nb, nu = R.workgroup_table_load(blocks, np.where(blocks >= 0, R.unit_of(blocks, R.dims(B, osh)["nsum"]), -1))
    form("crowded mark table", B, shape, n, table_load_max=int(nb.max()), table_slots=R.MARK_TAB_SLOTS)
    assert nb.max() > R.MARK_TAB_SLOTS and (nb[:-1] == 2048).all()
    out, osh, nbr = R.neighbours_strided(idx, B, shape, *geom)
    assert out.shape[0] == 8 * n
    W_out = R.grid_words(out, B, osh)
    idx_dev, n_dev = _dev(idx, cuda), S.device_scalar(n, cuda)
    grid, _ = build(idx_dev, n_dev, B, shape, keep_order=False)
    for counted in (True, False):
        monkeypatch.setattr(S, "COUNTED_MARKS", counted)
        s = strided(idx_dev, n_dev, grid, geom, out.shape[0] + 1)
        check_strided(f"crowded mark table counted={counted}", s, out, osh, nbr, W_out, counted=counted)


def test_crowded_count_table_of_the_strided_marks(cuda, monkeypatch):
    """A SHUFFLED row list on a grid without a permutation (the table then names ranks): the 256 rows of a workgroup come from all
    128 scenes and touch far more than 32 units of the wpw-1 output grid"""
    name, geom = "S4", (3, 2, (0, 1, 1))
    B, shape = GRIDS[name][:2]
    r = ref(name)
    idx, n = r["idx"], r["idx"].shape[0]      # (random row order)
    out, osh, nbr, W_out = ref_strided(name, geom)
    want = np.where(nbr >= 0, r["rank"][np.maximum(nbr, 0)], -1)     # no permutation: the entries are ranks
    nsum_out = R.dims(B, osh)["nsum"]
    blocks = R.output_blocks(idx, B, shape, *geom)
    _, nu = R.workgroup_table_load(blocks, np.where(blocks >= 0, R.unit_of(blocks, nsum_out), -1))
    form("crowded count table (strided)", B, osh, n, wpw_out=R.wpw(nsum_out), unit_load_min=int(nu.min()), unit_load_max=int(nu.max()), count_slots=R.CNT_TAB_SLOTS)
    assert R.wpw(nsum_out) == 1 and nu[:-1].min() > R.CNT_TAB_SLOTS
    idx_dev, n_dev = _dev(idx, cuda), S.device_scalar(n, cuda)
    grid, _ = build(idx_dev, n_dev, B, shape, keep_order=False)
    monkeypatch.setattr(S, "COUNTED_MARKS", True)
    s = strided(idx_dev, n_dev, grid, geom, out.shape[0] + 2)
    check_strided("crowded count table", s, out, osh, want, W_out, counted=True)


# ------------------------------------------------------------------------------------------------ (e) voxeliser
def _cells(points, b, cfg_args):
    """per-point (b, z, y, x) int64 and validity, in the kernel's arithmetic: f32 subtract, f32 divide, floor"""
    vs, rg = np.float32(cfg_args[0]), np.float32(cfg_args[1])
    grid = np.round((rg[3:] - rg[:3]) / vs).astype(np.int64)
    q = np.floor((points[:, :3] - rg[:3]) / vs)
    ok = ((q >= 0) & (q < grid.astype(np.float32))).all(1)
    c = np.where(ok[:, None], q, 0).astype(np.int64)
    return np.stack([np.full(points.shape[0], b, np.int64), c[:, 2], c[:, 1], c[:, 0]], 1), ok, [int(grid[2]), int(grid[1]), int(grid[0])]


def _unkey(key, gshape):
    """linear cell keys (ascending) -> (b, z, y, x)"""
    out = np.empty((key.shape[0], 4), np.int64)
    rem = key
    for d in (3, 2, 1):
        rem, out[:, d] = np.divmod(rem, gshape[d - 1])
    out[:, 0] = rem
    return out


def _vox_ref(scenes, cfg_args, oracle):
    vs, rg, C, mp, mv = cfg_args
    cs, ns, vx, ms, cells = [], [], [], [], []
    for b, p in enumerate(scenes):
        v, c, num = oracle.voxelize(p, vs, rg, mp, mv)
        cs.append(np.concatenate([np.full((c.shape[0], 1), b, np.int32), c], 1))
        ns.append(num)
        vx.append(v)
        ms.append(oracle.mean_vfe(v, num))
        cc, ok, gshape = _cells(p, b, cfg_args)
        cells.append(np.unique(((cc[ok, 1] * gshape[1] + cc[ok, 2]) * gshape[2] + cc[ok, 3]) + b * gshape[0] * gshape[1] * gshape[2]))
    return dict(coords=np.concatenate(cs), num_points=np.concatenate(ns), voxels=np.concatenate(vx), mean=np.concatenate(ms),
                cells=_unkey(np.concatenate(cells), gshape), gshape=gshape)


def _vox_run(scenes, cfg_args, cuda, grid_shape=None, grid=None):
    C = cfg_args[2]
    pts = np.concatenate(scenes, 0) if scenes else np.zeros((0, C), np.float32)
    off = np.zeros(len(scenes) + 1, np.int32)
    off[1:] = np.cumsum([p.shape[0] for p in scenes])
    cfg = S.make_voxel_cfg(*cfg_args)
    B = len(scenes)
    if grid is None:
        grid = S.alloc_grid(B, grid_shape or [cfg.grid[2], cfg.grid[1], cfg.grid[0]], cuda, with_perm_cap=max(pts.shape[0], 1))
    grid.perm.fill_(-2)
    return S.voxelize(_dev(pts, cuda), _dev(off, cuda), B, cfg, grid=grid, want_voxels=True)


def _check_vox(what, got, want, B):
    n, n_cells = int(got["n"].item()), int(got["n_cells"].item())
    assert n == want["coords"].shape[0], (what, n, want["coords"].shape[0])
    assert n_cells == want["cells"].shape[0], (what, n_cells, want["cells"].shape[0])
    R.compare_rows(f"{what}: coords in first-come order", got["coords"], want["coords"], n)
    for k in ("num_points", "voxels", "mean"):
        R.compare_rows(f"{what}: {k}", got[k], want[k], n)
    # the cells of voxels cut by max_voxels, listed behind the voxels in any order
    kept = {tuple(r) for r in want["coords"].tolist()}
    dropped = np.array(sorted(set(map(tuple, want["cells"].tolist())) - kept), np.int64).reshape(-1, 4)
    assert dropped.shape[0] == n_cells - n
    lost = got["coords"][n:n_cells].cpu().numpy().astype(np.int64)
    R.equal(f"{what}: dropped cells", lost[np.lexsort(lost.T[::-1])] if lost.size else lost, dropped)
    # the rank grid it leaves: all cells, perm = rank -> first-come row (-1 for a dropped cell and behind the cells)
    g = got["grid"]
    allc = np.concatenate([want["coords"].astype(np.int64), dropped])
    W = R.grid_words(allc, B, g.shape)
    check_words(f"{what}: rank grid", W, g, n_cells)
    perm = np.full(got["cap"], -1, np.int64)
    rank = R.rank_of(allc, B, g.shape)
    perm[rank[:n]] = np.arange(n)
    R.compare_rows(f"{what}: perm", g.perm[:got["cap"]], perm, got["cap"])
    return W, n, n_cells


SMALL_VOX = ([0.25, 0.25, 0.5], [-2.5, -2.5, -1.0, 2.5, 2.5, 1.0], 5, 3, 200)      # 20 x 20 x 4 cells


def _small_scene(rng, m):
    p = rng.uniform(-3, 3, size=(m, 5)).astype(np.float32)
    p[:, 2] = rng.uniform(-1.2, 1.2, size=m)
    return p


@pytest.mark.parametrize("empty", [False, True], ids=["all-filled", "edge-scenes-empty"])
@pytest.mark.parametrize("B", [63, 64, 65, 129])
def test_voxelize_many_scenes(cuda, oracle, monkeypatch, B, empty):
    """vox_scene_kernel walks the scenes 64 at a time with a running prefix; max_voxels = 200 cuts the scenes of more than 200
    cells (those of 400 points and more) and not the others"""
    rng = np.random.default_rng(B)
    hollow = {0, 63, 64, B - 1} if empty else set()
    scenes = [_small_scene(rng, 0 if b in hollow else int(rng.integers(150, 460))) for b in range(B)]
    scenes = [p if b % 7 else np.concatenate([p, np.full((3, 5), 50.0, np.float32)]) for b, p in enumerate(scenes)]     # (out-of-range points)
    want = _vox_ref(scenes, SMALL_VOX, oracle)
    per = np.bincount(want["coords"][:, 0], minlength=B)
    form(f"voxelize B={B}", B, want["gshape"], sum(p.shape[0] for p in scenes), scene_rounds=-(-B // R.SCENE_ROUND), cut_scenes=int((per == 200).sum()))
    assert (-(-B // R.SCENE_ROUND) > 1) == (B > 64) and (per == 200).any() and ((per > 0) & (per < 200)).any()
    got = _vox_run(scenes, SMALL_VOX, cuda)
    W, n, n_cells = _check_vox(f"B={B}", got, want, B)
    assert n_cells > n
    # dropped voxels: the summary-driven clear leaves zero; the row form leaves zero given the rows [0, n_cells)
    g = got["grid"]
    if empty:
        clear("summary", [(g, got["coords"], got["n_cells"])], monkeypatch)
    else:
        clear("row" if B % 2 else "rows", [(g, got["coords"], got["n_cells"])], monkeypatch)
    assert_zero(f"B={B} clear after dropped voxels", g)
    # ... and the cleared grid is as good as a fresh one: other points, counted prefix, word for word
    other = [_small_scene(rng, 300) for _ in range(B)]
    want2 = _vox_ref(other, SMALL_VOX, oracle)
    again, fresh = _vox_run(other, SMALL_VOX, cuda, grid=g), _vox_run(other, SMALL_VOX, cuda)
    _check_vox(f"B={B} on the cleared grid", again, want2, B)
    assert torch.equal(again["grid"].bits, fresh["grid"].bits) and torch.equal(again["grid"].summary, fresh["grid"].summary)
    assert torch.equal(again["grid"].counters, fresh["grid"].counters) and torch.equal(again["coords"][:int(again["n"].item())], fresh["coords"][:int(fresh["n"].item())])


@pytest.mark.parametrize("n", [256 * 4096, 256 * 4096 + 1, 257 * 4096 + 1])
def test_voxelize_many_points(cuda, oracle, n):
    """more than 256 scan tiles of 4 096 points: partial_scan_kernel carries between its rounds.  Scene 1 opens 600 points before
    the 257th tile, so that first points — whose first-come rank is that carry plus a tile prefix — lie on both sides of it.
    max_points 4 on 6 400 cells: nearly every cell is crowded (vox_crowded_insert_kernel)"""
    cfg_args = ([0.25, 0.25, 0.5], [-5.0, -5.0, -1.0, 5.0, 5.0, 1.0], 5, 4, 10000)
    rng = np.random.default_rng(n)
    split = 256 * R.SCAN_TILE - 600
    scenes = []
    for m in (split, n - split):
        p = rng.uniform(-5.2, 5.2, size=(m, 5)).astype(np.float32)
        p[:, 2] = rng.uniform(-1.1, 1.1, size=m)
        scenes.append(p)
    tiles = -(-n // R.SCAN_TILE)
    want = _vox_ref(scenes, cfg_args, oracle)
    cc, ok, _ = _cells(scenes[1], 1, cfg_args)
    key = np.where(ok, (cc[:, 1] * 64 + cc[:, 2]) * 64 + cc[:, 3], -1)
    late_firsts = int(R.first_flags(key)[600:].sum())       # first points of scene 1 at point 1 048 576 and later
    form(f"voxelize n={n}", 2, want["gshape"], n, scan_tiles=tiles, scan_rounds=-(-tiles // 256), first_points_behind_the_carry=late_firsts)
    assert tiles == {256 * 4096: 256, 256 * 4096 + 1: 257, 257 * 4096 + 1: 258}[n]
    assert late_firsts >= {256: 0, 257: 1, 258: 100}[tiles]      # (257 tiles: the one point of the last tile opens a voxel)
    assert (want["num_points"] == 4).mean() > 0.5
    got = _vox_run(scenes, cfg_args, cuda)
    _check_vox(f"n={n}", got, want, 2)


@pytest.mark.parametrize("B,w", [(2, 8), (12, 16)])
def test_voxelize_production_grid(cuda, oracle, monkeypatch, B, w):
    """syn.make_scene on the lidar grid through the counted marks (and the three-launch prefix) at wpw 8 and 16.  The rank grid is
    the backbone's [41, 1440, 1440] (one plane more than the voxel grid)"""
    args = (syn.VOXEL_SIZE, syn.POINT_CLOUD_RANGE, 5, 10, 160000)
    rng = np.random.default_rng(B)
    scenes = [syn.make_scene(10 + b) for b in range(B)]
    if B == 12:
        scenes[3] = scenes[3][rng.permutation(scenes[3].shape[0])]
        scenes[5] = scenes[5][:1].copy()
        scenes[8] = np.full((500, 5), 99.0, np.float32)
    want = _vox_ref(scenes, args, oracle)
    f = form(f"voxelize lidar B={B}", B, LIDAR, sum(p.shape[0] for p in scenes))
    assert f["wpw"] == w
    for counted in (True, False):
        monkeypatch.setattr(S, "COUNTED_MARKS", counted)
        got = _vox_run(scenes, args, cuda, grid_shape=LIDAR)
        W, n, n_cells = _check_vox(f"lidar B={B} counted={counted}", got, want, B)
        check_counters(f"lidar B={B} counted={counted}", W, got["grid"], counted)
        assert n == n_cells
    monkeypatch.setattr(S, "COUNTED_MARKS", True)
    clear("summary", [(got["grid"], got["coords"], got["n"])], monkeypatch)
    assert_zero("lidar: summary clear of an uncounted build", got["grid"])


def test_voxelize_crowded_count_table(cuda, oracle):
    """a SHUFFLED lidar scene on the one-scene grid (wpw 1): the 256 points of a marking workgroup touch far more than 32 units"""
    args = (syn.VOXEL_SIZE, syn.POINT_CLOUD_RANGE, 5, 10, 160000)
    rng = np.random.default_rng(3)
    p = syn.make_scene(4)
    p = p[rng.permutation(p.shape[0])]
    cc, ok, _ = _cells(p, 0, args)
    nsum = R.dims(1, LIDAR)["nsum"]
    blk = np.where(ok, R.block_and_bit(cc, 1, LIDAR)[0], -1)
    nb, nu = R.workgroup_table_load(blk, np.where(ok, R.unit_of(blk, nsum), -1))
    f = form("voxelize crowded count table", 1, LIDAR, p.shape[0], unit_load_min=int(nu.min()), unit_load_max=int(nu.max()), count_slots=R.CNT_TAB_SLOTS)
    assert f["wpw"] == 1 and nu[:-1].min() > R.CNT_TAB_SLOTS
    want = _vox_ref([p], args, oracle)
    got = _vox_run([p], args, cuda, grid_shape=LIDAR)
    W, _, _ = _check_vox("crowded count table", got, want, 1)
    check_counters("crowded count table", W, got["grid"], True)


def test_voxelize_scene_borders(cuda, oracle):
    """scene borders exactly on a scan tile (4 096), exactly on a workgroup (4 864 = 19 * 256), inside a wave at no multiple of 64
    (5 901 = 92 * 64 + 13), and an empty scene between"""
    rng = np.random.default_rng(11)
    sizes = [4096, 768, 1037, 0, 200, 64 * 3 + 1]
    off = np.cumsum([0] + sizes)
    assert off[1] % R.SCAN_TILE == 0 and off[2] % 256 == 0 and off[2] % R.SCAN_TILE and off[3] % 64 == 13
    scenes = [_small_scene(rng, m) for m in sizes]
    cfg_args = SMALL_VOX[:4] + (10000,)
    want = _vox_ref(scenes, cfg_args, oracle)
    form("voxelize scene borders", len(sizes), want["gshape"], int(off[-1]))
    _check_vox("scene borders", _vox_run(scenes, cfg_args, cuda), want, len(sizes))


# ------------------------------------------------------------------------------------------------ (f) clears
def _moved(name):
    """other coordinates for a second build: the grid's sites shifted by one cell in x (by -7 at the far face)"""
    k = (name, "moved")
    if k not in _REF:
        B, shape = GRIDS[name][:2]
        moved = ref(name)["idx"].copy()
        moved[:, 3] = np.where(moved[:, 3] + 1 < shape[2], moved[:, 3] + 1, moved[:, 3] - 7)
        moved = np.unique(moved, axis=0).astype(np.int32)
        _REF[k] = (moved, R.grid_words(moved, B, shape), R.rank_order(moved, B, shape))
    return _REF[k]


@pytest.mark.parametrize("kind", ["row", "rows", "summary"])
def test_clears_leave_grids_as_good_as_new(cuda, monkeypatch, kind):
    """three counted grids of the three prefix splits (wpw 1, 8, 16), cleared in one launch where the form allows: bits, summary
    and EVERY counter word are zero, and a second counted build with other coordinates equals one on a fresh grid word for word"""
    monkeypatch.setattr(S, "COUNTED_MARKS", True)
    jobs, second = [], []
    for name in ("G1", "G8", "G16"):
        B, shape, nsum, w, _, _ = GRIDS[name]
        r = ref(name)
        idx, n = r["idx"], r["idx"].shape[0]
        form(f"clear {kind} {name}", B, shape, n, counter_words=R.counter_words(nsum))
        idx_dev, n_dev = _dev(idx, cuda), S.device_scalar(n, cuda)
        grid, _ = build(idx_dev, n_dev, B, shape, keep_order=True)
        s = strided(idx_dev, n_dev, grid, (1, 1, 0), n)
        check_counters(f"{name} before the clear", r["W"], s.out_grid, True)
        jobs.append((s.out_grid, s.out_idx, s.out_n))
        second.append((name, grid, idx_dev, n_dev))
    clear(kind, jobs, monkeypatch)     # (rows / summary: the three grids in ONE launch)
    for (name, grid, idx_dev, n_dev), (og, _, _) in zip(second, jobs):
        assert_zero(f"{name} {kind}", og)
        # other coordinates: the layer (3, 2, 1)'s own inputs shifted by one cell in x where the grid allows
        B, shape = GRIDS[name][:2]
        moved, W2, perm2 = _moved(name)
        m_dev, mn_dev = _dev(moved, cuda), S.device_scalar(moved.shape[0], cuda)
        g2, _ = build(m_dev, mn_dev, B, shape, keep_order=True)
        a = strided(m_dev, mn_dev, g2, (1, 1, 0), moved.shape[0], out_grid=og)
        b = strided(m_dev, mn_dev, g2, (1, 1, 0), moved.shape[0])
        for what, s in (("cleared", a), ("fresh", b)):
            check_strided(f"{name} {kind} second build on the {what} grid", s, moved[perm2], list(shape), perm2[None, :], W2, counted=True)
        assert torch.equal(a.out_grid.bits, b.out_grid.bits) and torch.equal(a.out_grid.summary, b.out_grid.summary)
        assert torch.equal(a.out_grid.counters, b.out_grid.counters) and torch.equal(a.out_idx, b.out_idx) and torch.equal(a.nbr, b.nbr)
