"""Launch traces without a GPU: which entry points of the C ABI the host code calls, and with what.

Every kernel choice of `sparse.conv_forward` / `conv_forward_split` gives the same bits as the plain kernel by design, so no
result test can see a call that quietly takes another kernel.  Here the loaded library is replaced by a recorder
(`installed()`), the host code runs on CPU (or meta) tensors, and every call is written down: the trace of a fixed list of
cases is kept in tests/golden/launch_trace.json (written by tests/golden/make_launch_trace_golden.py) and
tests/test_launch_trace.py compares a fresh trace with it, entry for entry.

What is recorded of a call: the entry point's name and its arguments in order — scalars as they are, a tensor as
(shape, dtype, is PermutedWeight), NULL as None, a ConvGeom as its fifteen ints, a RankGridC as B, D, H, W and which of its
pointers are set, any other ctypes object (an array of pointers, a cast) as its type's name.  Size and count queries go to the
real library and are not recorded.  Only names that the product has had all along are used (attributes of a Rulebook are
assigned, never declared here), so the same file traces the code before and after a change of the host layer."""
import contextlib
import ctypes
import functools
import hashlib
import json
import os

import torch

from findnpropagate_amd import lib
from findnpropagate_amd import sparse as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_trace.json")


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _is_query(name):
    return name.endswith("_bytes") or name.startswith("fnp_rankgrid_num_") or name == "fnp_rankgrid_counter_words"


def _token(a):
    if a is None or isinstance(a, (bool, int, float, str)):
        return a
    if isinstance(a, tuple):       # (what the patched lib.ptr made of a tensor)
        return [list(a[0]), a[1], a[2]]
    if isinstance(a, lib.ConvGeom):
        return [int(v) for f in ("ksize", "stride", "padding", "in_shape", "out_shape") for v in getattr(a, f)]
    if isinstance(a, lib.RankGridC):
        return [a.B, a.D, a.H, a.W] + [bool(getattr(a, f)) for f in ("bits", "base", "summary", "perm", "counters")]
    if isinstance(a, (ctypes.Structure, ctypes.Array, ctypes._SimpleCData, ctypes._Pointer)):
        return type(a).__name__
    raise TypeError(f"launch trace: an argument of type {type(a).__name__} has no recorded form")


class Recorder:
    """stands in for the loaded library: queries go to the real one, every other fnp_* call returns 0 and is written down"""

    def __init__(self, real):
        self._real = real
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("fnp_"):
            raise AttributeError(name)
        if _is_query(name):
            return getattr(self._real, name)

        def call(*args):
            self.calls.append([name] + [_token(a) for a in args])
            return 0
        return call

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def _ptr(t):
    return None if t is None else (tuple(t.shape), _name(t.dtype), isinstance(t, S.PermutedWeight))


@contextlib.contextmanager
def installed():
    """the recorder in place of the library; the module switches that choose kernels at their defaults.  Everything is put back."""
    from findnpropagate_amd.backbones_3d import spconv_backbone as SB
    real = lib.load()
    rec = Recorder(real)
    saved = [(lib, n, getattr(lib, n)) for n in ("_lib", "require_device", "stream", "ptr")]
    saved += [(S, n, getattr(S, n)) for n in ("TILE_MODE", "ELL_MODE", "ELL_MFMA")] + [(SB, "TWO_STREAMS", SB.TWO_STREAMS)]
    try:
        lib._lib, lib.require_device, lib.stream, lib.ptr = rec, (lambda *t: None), (lambda: "stream"), _ptr
        S.TILE_MODE, S.ELL_MODE, S.ELL_MFMA, SB.TWO_STREAMS = None, None, True, None
        yield rec
    finally:
        for mod, name, value in saved:
            setattr(mod, name, value)


def _traced(rec, fn):
    """the calls of fn(); the lean refusal is part of the trace"""
    rec.take()
    try:
        fn()
    except lib.FnpError:
        return rec.take() + [["raise", "FnpError"]]
    return rec.take()


# ------------------------------------------------------------------------------------------------ (a) the operators
SHAPES = ((16, 16), (32, 32), (64, 64), (128, 128), (16, 32), (64, 128))
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
STATES = ("none", "tile_rb", "tile_rb+lean", "sorted", "rowmask", "perm_f32", "no_tile", "tile_rb+no_tile")
ROWS = 48


def _weight(K, cin, cout, dtype, permuted, device="cpu"):
    w = torch.empty((K, cout, cin), dtype=dtype, device=device)
    return w.as_subclass(S.PermutedWeight) if permuted else w


@functools.lru_cache(maxsize=None)
def _parts(K, cap, device, stride):
    """what the hand-made rulebooks are put together from (nothing writes into a tensor here: the cases share them)"""
    geom, _ = S.make_geom(3 if K == 27 else (3, 1, 1), 1, 1 if K == 27 else (1, 0, 0), [8, 8, 8], [8, 8, 8])
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=device)
    tiles = {c: torch.empty((int(lib.load().fnp_tile_rulebook_bytes(cap, c)),), dtype=torch.uint8, device=device) for c in S.TILED_CHANNELS}
    return geom, i32(K, stride), tiles, i32(cap), i32(cap // 16 + 1)


def _rulebook(K, cap, state, cin, device="cpu", stride=None):
    """a SubM rulebook made by hand, with the derived state of `state` planted as the product's own code leaves it"""
    geom, nbr, tiles, rows, blocks = _parts(K, cap, device, stride or cap)
    rb = S.Rulebook(nbr=nbr, K=K, cap_out=cap, geom=geom)
    for part in state.split("+"):
        if part == "tile_rb":
            rb._tile_rb = dict(tiles)
        elif part == "lean":
            rb._lean = True
        elif part == "sorted":
            rb._sorted = (rows, blocks)
        elif part == "rowmask":
            rb._rowmask = rows
        elif part == "perm_f32":
            rb._perm_f32 = {cin: rows}
        elif part == "no_tile":
            rb._no_tile = True
        else:
            assert part == "none", part
    return rb


def _forward(split, feat, w, rb, n, out_dtype=None, ranked=False, tile=None, valu=False):
    if split:
        return S.conv_forward_split(feat, w, rb, n, ranked=ranked, tile=tile)
    return S.conv_forward(feat, w, rb, n, out_dtype=out_dtype, ranked=ranked, tile=tile, valu=valu)


def operator_cases(rec):
    n = torch.empty((1,), dtype=torch.int32)
    for split in (False, True):
        for K in (27, 3):
            for cin, cout in SHAPES:
                for dtype in DTYPES[:2] if split else DTYPES:
                    f32 = dtype == torch.float32
                    feat = torch.empty((ROWS, cin), dtype=dtype)
                    for permuted in (False, True) if f32 else (False,):
                        w = _weight(K, cin, cout, dtype, permuted)
                        for out_dtype in (None,) if split else (None, torch.float32):
                            for ranked in (False, True):
                                for tile in (None, True, False):
                                    for valu in (False, True) if f32 else (False,):
                                        for mode in (None, True, False):
                                            for state in STATES:
                                                S.TILE_MODE = mode
                                                rb = _rulebook(K, ROWS, state, cin)
                                                cid = (f"{'split' if split else 'forward'} K{K} {cin}>{cout} {_name(dtype)}{' permuted' if permuted else ''}"
                                                       f" out={out_dtype and _name(out_dtype)} ranked={ranked} tile={tile} valu={valu} TILE_MODE={mode} {state}")
                                                yield cid, _traced(rec, lambda: _forward(split, feat, w, rb, n, out_dtype, ranked, tile, valu))
    S.TILE_MODE = None


LIMIT = 0x7fffffff


def limit_cases(rec):
    """the 32-bit-offset fall-backs, one row below and at each limit; meta tensors: no memory"""
    n = torch.empty((1,), dtype=torch.int32, device="meta")

    def one(cid, split, rows, cin, dtype, state, permuted=False, stride=None, tile=None):
        feat = torch.empty((rows, cin), dtype=dtype, device="meta")
        w = _weight(27, cin, cin, dtype, permuted, "meta")
        rb = _rulebook(27, ROWS, state, cin, "meta", stride=stride)
        return f"{cid} {'split' if split else 'forward'} rows={rows} stride={stride or ROWS}", _traced(rec, lambda: _forward(split, feat, w, rb, n, ranked=True, tile=tile))

    def first_over(bytes_per_row):
        return -(-LIMIT // bytes_per_row)      # the smallest row count with rows * bytes_per_row >= LIMIT

    for split in (False, True):
        for rows in (first_over(64 * 2) - 1, first_over(64 * 2)):
            yield one("tiled features", split, rows, 64, torch.bfloat16, "tile_rb", tile=True)
        for rows in (first_over(128 * 2) - 1, first_over(128 * 2)):
            yield one("sorted features", split, rows, 128, torch.bfloat16, "sorted")
        for stride in (first_over(27 * 4) - 1, first_over(27 * 4)):
            yield one("tiled table", split, ROWS, 64, torch.bfloat16, "tile_rb", stride=stride, tile=True)
    for permuted in (False, True):
        for rows in (first_over(128 * 4) - 1, first_over(128 * 4)):
            yield one(f"f32 sorted features{' permuted' if permuted else ''}", False, rows, 128, torch.float32, "perm_f32", permuted)
    for cin in (16, 128):
        for rows in (first_over(cin * 4) - 1, first_over(cin * 4)):
            yield one(f"permuted weight {cin}", False, rows, cin, torch.float32, "none", True)


def ell_cases(rec):
    n = torch.empty((1,), dtype=torch.int32)
    for ell_mfma in (True, False):
        for mfma in (None, True, False):
            for cin, cout in sorted(S.ELL_SHAPES):
                for dtype in DTYPES:
                    for out_dtype in (None, torch.float32):
                        S.ELL_MFMA = ell_mfma
                        rb = _rulebook(27, ROWS, "none", cin)
                        rb._ell = (torch.empty((ROWS * 8 + 64,), dtype=torch.int32), 8, torch.empty((1,), dtype=torch.int32))
                        feat, w = torch.empty((ROWS, cin), dtype=dtype), _weight(27, cin, cout, dtype, False)
                        yield (f"ell {cin}>{cout} {_name(dtype)} out={out_dtype and _name(out_dtype)} mfma={mfma} ELL_MFMA={ell_mfma}",
                               _traced(rec, lambda: S.conv_forward_ell(feat, w, rb, n, out_dtype=out_dtype, mfma=mfma)))
    S.ELL_MFMA = True


# ------------------------------------------------------------------------------------------------ (b) the backward's choice
def backward_cases(rec):
    from findnpropagate_amd.spconv.conv import SparseConvFunction
    n = torch.empty((1,), dtype=torch.int32)

    def step(feats, weight, rb, n_out, n_in, ranked):
        out = SparseConvFunction.apply(feats, weight, rb, n_out, n_in, ranked)
        out.backward(torch.zeros_like(out))

    def tensors(rows, cin, cout, ks, dtype):
        return (torch.zeros((rows, cin), dtype=dtype, requires_grad=True), torch.zeros((cout, *ks, cin), requires_grad=True))

    for C in (32, 64, 128):
        for dtype in (torch.bfloat16, torch.float32):
            for ranked in (False, True):
                for state in ("none", "sorted"):
                    feats, weight = tensors(ROWS, C, C, (3, 3, 3), dtype)
                    rb = _rulebook(27, ROWS, state, C)
                    yield f"subm {C} {_name(dtype)} ranked={ranked} {state}", _traced(rec, lambda: step(feats, weight, rb, n, n, ranked))
    # a strided layer (out_indices set): the transposed table, made once and kept with the rulebook — the second step reuses it
    for dtype in (torch.bfloat16, torch.float32):
        feats, weight = tensors(ROWS, 32, 64, (3, 3, 3), dtype)
        rb = _rulebook(27, 2 * ROWS, "none", 32)
        rb.out_indices, rb.out_n = torch.empty((2 * ROWS, 4), dtype=torch.int32), n
        for visit in (1, 2):
            yield f"strided 32>64 {_name(dtype)} visit {visit}", _traced(rec, lambda: step(feats, weight, rb, n, n, False))
    # an even kernel size is not its own mirror: the transposed table although the rows are the input's
    feats, weight = tensors(ROWS, 32, 32, (2, 2, 2), torch.bfloat16)
    geom, _ = S.make_geom(2, 1, 0, [8, 8, 8], [8, 8, 8])
    rb = S.Rulebook(nbr=torch.empty((8, ROWS), dtype=torch.int32), K=8, cap_out=ROWS, geom=geom)
    yield "even kernel 32 bfloat16 ranked=True", _traced(rec, lambda: step(feats, weight, rb, n, n, True))


# ------------------------------------------------------------------------------------------------ (c) the engine
ENGINE_VARIANTS = ("default", "tile_off", "rulebook_log", "ELL_MODE=False", "ELL_MODE=True ELL_MFMA=False", "TILE_MODE=False")


def engine_cases(rec):
    """FusedResBackbone.run(sync=False) on CPU tensors: the whole forward's launches.  3,000 rows: the tiled stages run and
    nothing is sorted; 131,072: stage 4 reaches SORT_MIN_ROWS and every stage of the f32 engine F32_SORT_MIN_ROWS."""
    from findnpropagate_amd.backbones_3d import spconv_backbone as SB
    for fnp_dtype in ("bf16", "fp16", "fp32", "bf16x3"):
        module = SB.VoxelResBackBone8x({"USE_BIAS": False, "FNP_DTYPE": fnp_dtype}, 5, [64, 64, 8]).eval()
        for cap1 in (3000, 131072):
            feats, idx = torch.empty((cap1, 5), dtype=torch.float32), torch.empty((cap1, 4), dtype=torch.int32)
            n1 = torch.empty((1,), dtype=torch.int32)
            for variant in ENGINE_VARIANTS:
                if fnp_dtype == "bf16x3" and variant == "rulebook_log":
                    continue      # (the engine refuses the hook: a bf16x3 layer is several launches)
                eng = SB.FusedResBackbone(module)
                S.TILE_MODE, S.ELL_MODE, S.ELL_MFMA = None, None, True
                if variant == "tile_off":
                    eng.tile_off = {0: 5}
                elif variant == "rulebook_log":
                    eng.rulebook_log = []
                elif variant == "ELL_MODE=False":
                    S.ELL_MODE = False
                elif variant == "ELL_MODE=True ELL_MFMA=False":
                    S.ELL_MODE, S.ELL_MFMA = True, False
                elif variant == "TILE_MODE=False":
                    S.TILE_MODE = False
                yield f"engine {fnp_dtype} cap1={cap1} {variant}", _traced(rec, lambda: eng.run(feats, idx, n1, 1, sync=False))
    S.TILE_MODE, S.ELL_MODE, S.ELL_MFMA = None, None, True


# ------------------------------------------------------------------------------------------------ (d) the engine under capture
class _Word:
    """stands in for a tensor the counts launch is handed by address: the pinned counts (there is no pinned memory without a
    device) or the device word behind them"""

    def __init__(self, words, cuda):
        self.shape, self.dtype, self.is_cuda = (words,), torch.int32, cuda

    def is_pinned(self):
        return not self.is_cuda

    def numel(self):
        return self.shape[0]

    def data_ptr(self):
        return 0

    def is_contiguous(self):
        return True


class _Capture:
    """stands in for the _PointsGraph being captured: what the engine reads of it, and its two cuts written into the trace
    where the engine makes them"""

    def __init__(self, rec, probe, split_index):
        self._rec, self.probe, self.host_counts, self.split_index, self.deferred = rec, probe, not probe, split_index, []
        self.counts_pin, self.counts_seq = _Word(32, False), _Word(1, True)

    def counts_ready(self, counts_dev):
        self._rec.calls.append(["cut", "counts"])

    def index_ready(self):
        self._rec.calls.append(["cut", "index"])


def engine_capture_cases(rec):
    """FusedResBackbone._run_once as a _PointsGraph calls it while it captures, in its four forms: one graph with host counts,
    the two-graph probe form, and each of them with the index chain a graph of its own.  Behind the forward's own launches,
    after a ["deferred"] marker: the launches the probe form hands over for replay()."""
    from findnpropagate_amd.backbones_3d import spconv_backbone as SB

    def forward(eng, cap, feats, idx, n1):
        eng._run_once(feats, idx, n1, 1, None, False, None, None, cap)
        rec.calls.append(["deferred"])
        for _, launch in cap.deferred:
            launch()

    for fnp_dtype in ("bf16", "fp16", "fp32", "bf16x3"):
        module = SB.VoxelResBackBone8x({"USE_BIAS": False, "FNP_DTYPE": fnp_dtype}, 5, [64, 64, 8]).eval()
        for cap1 in (3000, 131072):
            feats, idx = torch.empty((cap1, 5), dtype=torch.float32), torch.empty((cap1, 4), dtype=torch.int32)
            n1 = torch.empty((1,), dtype=torch.int32)
            for probe, split in ((False, False), (False, True), (True, False), (True, True)):
                if fnp_dtype == "bf16x3" and probe:
                    continue      # (the engine refuses: the deferred launches are written for the one-launch engines)
                eng, cap = SB.FusedResBackbone(module), _Capture(rec, probe, split)
                yield (f"capture {fnp_dtype} cap1={cap1} two_graphs={probe} split_index={split}",
                       _traced(rec, lambda: forward(eng, cap, feats, idx, n1)))


SECTIONS = {"operator": operator_cases, "limits": limit_cases, "ell": ell_cases, "backward": backward_cases, "engine": engine_cases,
            "engine_capture": engine_capture_cases}


# ------------------------------------------------------------------------------------------------ the fixture
def _ids_digest(ids):
    return hashlib.sha256("\n".join(ids).encode()).hexdigest()


def record(section):
    """(ids, traces) of one section, traced now"""
    with installed() as rec:
        ids, traces = [], []
        for cid, calls in SECTIONS[section](rec):
            ids.append(cid)
            traces.append(calls)
    assert len(set(ids)) == len(ids)
    return ids, traces


def dump(path=GOLDEN):
    """every section into one JSON file: a table of the distinct calls, one per line, and per case the numbers of its calls.
    The ten thousands of operator cases are named by the digest of their ids, the other sections case by case."""
    table, lines, sections = {}, [], {}
    for section in SECTIONS:
        ids, traces = record(section)
        rows = []
        for calls in traces:
            row = []
            for call in calls:
                key = json.dumps(call, separators=(",", ":"))
                if key not in table:
                    table[key] = len(lines)
                    lines.append(key)
                row.append(table[key])
            rows.append(row)
        sections[section] = {"cases": len(ids), "ids_sha256": _ids_digest(ids), "calls_of_case": rows}
        if len(ids) <= 1000:
            sections[section]["ids"] = ids
    with open(path, "w") as f:
        f.write('{"calls":[\n' + ",\n".join(lines) + '\n],\n"sections":{\n')
        f.write(",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'), sort_keys=True)}" for k, v in sections.items()))
        f.write("\n}}\n")


def load(path=GOLDEN):
    with open(path) as f:
        return json.load(f)
