"""A plain CPU reference for the BOX operators at the sizes where their kernels change form: inputs with a fixed seed, the pairs
that can overlap at all, the axis-aligned suppression mask restated in float32 numpy, the rotated IoU of the CPU oracle on the
candidate pairs, the reference's greedy sweep over a u64 mask, and views of the device workspace as such masks.  A helper module,
not a fixture, in the manner of ref_index.py and ref64.py; everything here runs on the CPU.

THE MASK (iou3d_nms_kernel.cu:306-323, :367-384).  n score-sorted boxes, cb = ceil(n / 64) column words: word [i, w] bit b is
set iff box j = 64 w + b comes after i and IoU(i, j) > thresh.  The sweep (iou3d_nms.cpp:139-155) walks i upwards, keeps i unless
its bit is set in remv, and ORs row i's words w >= i // 64 into remv.  Only words at or right of the diagonal are ever read; the
reference's kernel fills the tiles left of it too, csrc/iou3d_nms.hip leaves them 0.

THE INPUTS (make_boxes).  nc = n // 6 cluster centres (x, y in +-60 m, sizes 0.5 to 8 m, headings in +-pi), members = centre +
normal noise of scale NOISE, sizes clamped to >= 0.5 m, rows "heads first": rows 0 .. nc-1 hold one member of each cluster, the
rest are shuffled behind, so that suppressors sit in the early words and the suppressed boxes in the late ones.  Planted on top
(n >= 256): rows 0 .. 7 are EXACT heads — heading 0, every other field a multiple of 1/4 — and the last 8 rows are their exact
duplicates, row n-1 that of row 0; rows 8 .. 12 carry the headings 0, +-pi/2, +-pi; rows 13 / n-10 touch along an edge, rows
14 / n-9 are nested (both pairs stand apart from the clusters).  Row 0 is always kept, so its duplicate in the last word has one
kept suppressor only, in word 0: at n = 4161 that is the one box 65 words away, at n = 4097 the one exactly 64 words away.

WHICH PAIRS CAN OVERLAP (candidates).  Pairs i < j whose centre distance (float64) is at most hypot(dx, dy) / 2 of both boxes plus
0.1 m.  Any other pair is separated by more than the two circumradii plus ten times the 1e-2 corner margin: no edge crossing, no
corner inside, overlap 0 in any arithmetic, bit 0 in both NMS flavours, no allowance.  The oracle is evaluated on candidates only.

BAND.  The CPU oracle evaluates cosf / sinf / atan2f with libm, the device with ocml, so a rotated IoU within rounding of the
threshold may fall on either side.  The width is MEASURED against the oracle (heading_sensitivity): the largest change of the
oracle's IoU over the candidate pairs when every heading is moved by 4 float32 ulps — up, down, and the two boxes of a pair in
opposite senses —, which models several ulps of error in cosf / sinf, times 4 as a margin.  Measured on the CPU on the inputs of
tests/test_gpu_box_at_scale.py (SEED 4), with the undecided pairs |IoU - thresh| < BAND as a share of the pairs over the threshold:

      n   candidates   max |dIoU|, 4 ulps    x 4        undecided / over at 0.1     at 0.7
    4096      88 830       1.657e-05       6.63e-05     20 / 26 226 = 0.076 %    2 / 3 855 = 0.052 %
    4097      86 911       1.878e-05       7.51e-05     18 / 26 532 = 0.068 %    7 / 4 036 = 0.173 %
    4161      89 847       1.466e-05       5.87e-05     16 / 27 377 = 0.058 %    2 / 4 090 = 0.049 %
    4800     120 358       1.472e-05       5.89e-05     33 / 35 417 = 0.093 %    4 / 4 992 = 0.080 %

so BAND = 8e-5, the largest product rounded up, and the shares stay far under the cap of 0.5 %; at threshold 1.0 (n = 4161) no pair
is over or undecided.  tests/test_ref_box.py recomputes the figures and holds 4 x measured <= BAND for every size, and for the
pairwise (4.8e-06, aligned 1.7e-05) and recall (6.3e-06 on the 3-D IoU) inputs too.  The measurement is about THESE inputs: in about
one draw in three some pair sits on a discontinuity of the reference's algorithm (a corner entering the 1e-2 margin, an edge
crossing appearing) where 4 ulps move the IoU by 3e-4 to 4e-3; the seed is one whose four draws hold no such pair, which the CPU
test asserts.

A pair whose two headings are both exactly 0 is never undecided: cosf(0) = 1 and sinf(0) = 0 exactly in any library, so the IEEE
operation sequence gives the same bits on both sides.  That is what lets threshold 1.0 be checked on the exact duplicates, whose
IoU is exactly 1.0 and therefore not "> 1.0".
"""
import functools
import hashlib

import numpy as np

SEED = 4
NOISE = np.array([0.3, 0.3, 0.1, 0.2, 0.2, 0.1, 0.15])
N_EXACT = 8                      # exact heads (rows 0 .. 7) and their duplicates (the last 8 rows)
EXACT_HEADINGS = (0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi)
BAND = 8.0e-5                    # |IoU - thresh| below which a rotated bit is undecided between libm and ocml (measured: see above)
UNDECIDED_SHARE_CAP = 0.005      # of the pairs over the threshold



def words(n):
    return (int(n) + 63) // 64


# ------------------------------------------------------------------------------------------------------------------ inputs
def clustered(r, n, spread=60.0):
    """n clustered boxes, heads first, without planted rows"""
    nc = max(n // 6, 1)
    c = np.empty((nc, 7))
    c[:, 0:2] = r.uniform(-spread, spread, (nc, 2))
    c[:, 2] = r.uniform(-2.0, 1.0, nc)
    c[:, 3:6] = r.uniform(0.5, 8.0, (nc, 3))
    c[:, 6] = r.uniform(-np.pi, np.pi, nc)
    cid = np.concatenate([np.arange(min(nc, n)), r.permutation(np.arange(max(n - nc, 0)) % nc)])
    b = c[cid] + r.normal(size=(n, 7)) * NOISE
    b[:, 3:6] = np.maximum(b[:, 3:6], 0.5)
    return b.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _make_boxes(n, seed):
    r = np.random.default_rng([seed, n])
    b = clustered(r, n)
    if n >= 256:
        q = b[:N_EXACT].astype(np.float64)
        q = np.round(q * 4) / 4
        q[:, 3:6] = np.maximum(q[:, 3:6], 0.5)
        q[:, 6] = 0.0
        b[:N_EXACT] = q
        for k, h in enumerate(EXACT_HEADINGS):
            b[N_EXACT + k, 6] = np.float32(h)
        b[13] = [100, 100, 0, 4, 2, 1, 0.0]
        b[n - 10] = [104, 100, 0, 4, 2, 1, 0.0]                       # touches row 13 along an edge
        b[14] = [100, -100, 0, 10, 10, 1, 0.2]
        b[n - 9] = [100.5, -100.3, 0, 1.5, 0.7, 1, 1.1]               # nested in row 14
        b[n - N_EXACT:] = b[:N_EXACT][::-1]                           # row n-1 duplicates row 0
    b.setflags(write=False)
    return b


def make_boxes(n, seed=SEED):
    """(n, 7) float32 score-sorted boxes of the at-scale NMS cases (read-only, shared)"""
    return _make_boxes(int(n), int(seed))


def duplicate_pairs(n):
    """(8, 2) rows (head, its exact duplicate)"""
    return np.array([[k, n - 1 - k] for k in range(N_EXACT)], np.int64)


# ------------------------------------------------------------------------------------------------------------------ pairs
_CAND = {}


def candidates(boxes):
    """(m, 2) int64 pairs i < j that can overlap at all, in row-major order (computed once per input)"""
    boxes = np.ascontiguousarray(boxes, np.float32)
    key = hashlib.sha1(boxes.tobytes()).hexdigest()
    if key not in _CAND:
        b = boxes.astype(np.float64)
        n = b.shape[0]
        rad = np.hypot(b[:, 3], b[:, 4]) / 2
        out = [np.zeros((0, 2), np.int64)]
        for i0 in range(0, n, 512):
            i1 = min(i0 + 512, n)
            d = np.hypot(b[i0:i1, None, 0] - b[None, :, 0], b[i0:i1, None, 1] - b[None, :, 1])
            ii, jj = np.nonzero(d <= rad[i0:i1, None] + rad[None, :] + 0.1)
            ii += i0
            m = ii < jj
            out.append(np.stack([ii[m], jj[m]], 1))
        p = np.concatenate(out)
        p.setflags(write=False)
        _CAND[key] = p
    return _CAND[key]


def iou_rotated(boxes, pairs):
    """float32 BEV IoU of the CPU oracle on `pairs`: its overlap, then ov / max(sa + sb - ov, 1e-8) as iou3d_nms_kernel.cu:227-234"""
    from oracle import oracle as O

    boxes = np.ascontiguousarray(boxes, np.float32)
    a, b = boxes[pairs[:, 0]], boxes[pairs[:, 1]]
    ov = O.boxes_aligned_overlap_bev(a, b)
    sa, sb = a[:, 3] * a[:, 4], b[:, 3] * b[:, 4]
    return ov / np.maximum(sa + sb - ov, np.float32(1e-8))


def _ulps(h, k):
    h = np.array(h, np.float32)
    for _ in range(abs(k)):
        h = np.nextafter(h, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return h


def heading_sensitivity(boxes, pairs, iou_fn=None, ulps=4):
    """max |IoU' - IoU| over `pairs` when every heading moves by `ulps` float32 ulps: both boxes up, both down, and in opposite
    senses.  A heading of exactly 0 stays (its trigonometry is exact).  iou_fn(a, b) -> per-pair IoU, default the oracle's BEV IoU."""
    boxes = np.ascontiguousarray(boxes, np.float32)
    if iou_fn is None:
        def iou_fn(a, b):
            both = np.concatenate([a, b])
            k = a.shape[0]
            return iou_rotated(both, np.stack([np.arange(k), np.arange(k) + k], 1))
    a, b = boxes[pairs[:, 0]], boxes[pairs[:, 1]]
    base = iou_fn(a, b)
    worst = 0.0
    for sa, sb in ((1, 1), (-1, -1), (1, -1), (-1, 1)):
        a2, b2 = a.copy(), b.copy()
        a2[:, 6] = np.where(a[:, 6] == 0, a[:, 6], _ulps(a[:, 6], sa * ulps))
        b2[:, 6] = np.where(b[:, 6] == 0, b[:, 6], _ulps(b[:, 6], sb * ulps))
        worst = max(worst, float(np.abs(iou_fn(a2, b2) - base).max(initial=0.0)))
    return worst


def undecided(boxes, pairs, iou, thresh):
    """bool per pair: within BAND of the threshold, unless both headings are exactly 0 (no trigonometric rounding at all)"""
    exact = (boxes[pairs[:, 0], 6] == 0) & (boxes[pairs[:, 1], 6] == 0)
    return (np.abs(iou.astype(np.float64) - np.float64(np.float32(thresh))) < BAND) & ~exact


# ------------------------------------------------------------------------------------------------------------------ masks
def pack_bits(flags):
    """(n, m) bool -> (n, ceil(m / 64)) uint64, bit b of word w = column 64 w + b"""
    n, m = flags.shape
    cb = words(m)
    pad = np.zeros((n, cb * 64), bool)
    pad[:, :m] = flags
    return np.packbits(pad, axis=1, bitorder="little").view("<u8").astype(np.uint64).reshape(n, cb)


def get_bits(mask, pairs):
    """bit (i, j) of a (n, cb) uint64 mask for every pair"""
    i, j = pairs[:, 0], pairs[:, 1]
    return ((mask[i, j >> 6] >> (j & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


def mask_from_pairs(n, pairs, flags):
    """(n, cb) uint64 mask with bit (i, j) set for the pairs whose flag is True"""
    m = np.zeros((n, words(n)), np.uint64)
    p = pairs[np.asarray(flags, bool)]
    np.bitwise_or.at(m, (p[:, 0], p[:, 1] >> 6), np.uint64(1) << (p[:, 1] & 63).astype(np.uint64))
    return m


def upper_words(n):
    """(n, cb) bool: the words at or right of the diagonal, the ones the sweep reads"""
    return np.arange(words(n))[None, :] >= (np.arange(n) // 64)[:, None]


def mask_normal(boxes, thresh, ge=False):
    """The axis-aligned suppression mask in float32 numpy: iou3d_nms_kernel.cu:327-338 in the operation order of iou_axis_aligned,
    bit (i, j) = j > i and IoU > thresh.  No trigonometry: the device mask must equal it bit for bit.  (ge: the planted defect
    ">= thresh" of tests/test_ref_box.py.)"""
    b = np.ascontiguousarray(boxes, np.float32)
    n = b.shape[0]
    two = np.float32(2)
    lo_x, hi_x = b[:, 0] - b[:, 3] / two, b[:, 0] + b[:, 3] / two
    lo_y, hi_y = b[:, 1] - b[:, 4] / two, b[:, 1] + b[:, 4] / two
    area = b[:, 3] * b[:, 4]
    t = np.float32(thresh)
    out = np.zeros((n, words(n)), np.uint64)
    col = np.arange(n)
    for i0 in range(0, n, 512):
        s = slice(i0, min(i0 + 512, n))
        left, right = np.maximum(lo_x[s, None], lo_x[None, :]), np.minimum(hi_x[s, None], hi_x[None, :])
        top, bottom = np.maximum(lo_y[s, None], lo_y[None, :]), np.minimum(hi_y[s, None], hi_y[None, :])
        w, h = np.maximum(right - left, np.float32(0)), np.maximum(bottom - top, np.float32(0))
        inter = w * h
        iou = inter / np.maximum(area[s, None] + area[None, :] - inter, np.float32(1e-8))
        assert iou.dtype == np.float32
        out[s] = pack_bits((iou >= t if ge else iou > t) & (col[None, :] > col[s, None]))
    return out


def host_sweep(mask, n):
    """The reference's greedy sweep (iou3d_nms.cpp:139-155) over a (n, ceil(n / 64)) uint64 mask -> kept rows, int64.  Only the
    words at or right of the diagonal are read."""
    mask = np.asarray(mask, np.uint64).reshape(n, words(n)) if n else np.zeros((0, 0), np.uint64)
    remv = np.zeros((words(n),), np.uint64)
    keep = []
    one = np.uint64(1)
    for i in range(n):
        w = i >> 6
        if not (remv[w] >> np.uint64(i & 63)) & one:
            keep.append(i)
            remv[w:] |= mask[i, w:]
    return np.array(keep, np.int64)


def decode_ws(ws, n):
    """the workspace fnp_nms_rotated / fnp_nms_normal leave behind (bytes or u64 words, host array) as a (n, cb) uint64 mask"""
    w = np.ascontiguousarray(ws).view(np.uint64).reshape(-1)
    return w[: n * words(n)].reshape(n, words(n)).copy()


def decode_ws_batched(ws, cap, counts):
    """the workspace of fnp_nms_batched as one mask per list: list z starts at z * cap * ceil(cap / 64) words and its row stride is
    that of its OWN count, ceil(min(counts[z], cap) / 64)"""
    w = np.ascontiguousarray(ws).view(np.uint64).reshape(-1)
    out = []
    for z, c in enumerate(counts):
        c = min(int(c), cap)
        base = z * cap * words(cap)
        out.append(w[base: base + c * words(c)].reshape(c, words(c)).copy())
    return out


# ------------------------------------------------------------------------------------------------------------------ cases and checkers
NMS_SIZES = (4096, 4097, 4161, 4800)        # 64 words (the workload's size) | 65, the last holding one row | 66: the first second
NMS_CASES = tuple((n, t) for n in NMS_SIZES for t in (0.1, 0.7)) + ((4161, 1.0),)     # trip of the update loop | 75 words


@functools.lru_cache(maxsize=None)
def rotated_pairs(n):
    """boxes, candidate pairs and the oracle's IoU on them, once per size"""
    boxes = make_boxes(n)
    pairs = candidates(boxes)
    iou = iou_rotated(boxes, pairs)
    iou.setflags(write=False)
    return boxes, pairs, iou


@functools.lru_cache(maxsize=None)
def rotated_case(n, thresh):
    """what the CPU oracle says about a rotated case: over / undecided flags per candidate pair, its mask and its keep list"""
    boxes, pairs, iou = rotated_pairs(n)
    over = iou > np.float32(thresh)
    und = undecided(boxes, pairs, iou, thresh)
    mask = mask_from_pairs(n, pairs, over)
    keep = host_sweep(mask, n)
    return dict(n=n, thresh=thresh, boxes=boxes, pairs=pairs, iou=iou, over=over, undecided=und, mask=mask, keep=keep)


@functools.lru_cache(maxsize=None)
def normal_case(n, thresh):
    boxes = make_boxes(n)
    mask = mask_normal(boxes, thresh)
    return dict(n=n, thresh=thresh, boxes=boxes, pairs=candidates(boxes), mask=mask, keep=host_sweep(mask, n))


def check_mask_shape(mask, n, pairs):
    """findings of a (n, cb) mask that hold for both flavours: bits outside the candidate pairs, bits of columns past n"""
    allowed = mask_from_pairs(n, pairs, np.ones((len(pairs),), bool))
    out = dict(non_candidate=int(np.count_nonzero(mask & ~allowed)), past_n=0)
    if n % 64:
        out["past_n"] = int(np.count_nonzero(mask[:, -1] >> np.uint64(n % 64)))
    return out


def check_mask_rotated(mask, case):
    """findings of a rotated mask against the oracle: candidate bits that differ although the pair is decided"""
    out = check_mask_shape(mask, case["n"], case["pairs"])
    diff = get_bits(mask, case["pairs"]) != case["over"]
    out["decided_wrong"] = int(np.count_nonzero(diff & ~case["undecided"]))
    out["undecided_differ"] = int(np.count_nonzero(diff & case["undecided"]))
    return out


def check_mask_normal(mask, case):
    out = check_mask_shape(mask, case["n"], case["pairs"])
    up = upper_words(case["n"])
    out["words_differ"] = int(np.count_nonzero((mask != case["mask"]) & up))
    return out


# ------------------------------------------------------------------------------------------------------------------ sweeps' structure
def kept_suppressions(mask, keep, n):
    """(m, 2) pairs (i, j): i kept, j > i, bit (i, j) set — every suppression the sweep applies"""
    keep = np.asarray(keep, np.int64)
    bits = np.unpackbits(np.ascontiguousarray(mask[keep]).view(np.uint8), axis=1, bitorder="little")[:, :n]
    r, j = np.nonzero(bits)
    i = keep[r]
    m = j > i
    return np.stack([i[m], j[m]], 1)


def nearest_suppressor_words(mask, keep, n):
    """per box j the distance in WORDS to its nearest kept suppressor, -1 where it has none, and the distances of all suppressions"""
    s = kept_suppressions(mask, keep, n)
    d = (s[:, 1] >> 6) - (s[:, 0] >> 6)
    near = np.full((n,), np.iinfo(np.int64).max, np.int64)
    np.minimum.at(near, s[:, 1], d)
    near[near == np.iinfo(np.int64).max] = -1
    return near, d


# ------------------------------------------------------------------------------------------------------------------ 3-D IoU
def _iou3d(a, b, ov):
    two = np.float32(2)
    a_max, a_min = a[..., 2] + a[..., 5] / two, a[..., 2] - a[..., 5] / two
    b_max, b_min = b[..., 2] + b[..., 5] / two, b[..., 2] - b[..., 5] / two
    oh = np.maximum(np.minimum(a_max, b_max) - np.maximum(a_min, b_min), np.float32(0))
    o3 = ov * oh
    va, vb = a[..., 3] * a[..., 4] * a[..., 5], b[..., 3] * b[..., 4] * b[..., 5]
    out = o3 / np.maximum(va + vb - o3, np.float32(1e-6))
    assert out.dtype == np.float32
    return out


def iou3d_from_overlap(a, b, ov):
    """boxes_iou3d_gpu (iou3d_nms_utils.py:59-80) from a given BEV overlap, float32 numpy: a (N, 7), b (M, 7) and ov (N, M), or the
    aligned form a, b (N, 7) and ov (N,)"""
    a, b, ov = np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(ov, np.float32)
    return _iou3d(a, b, ov) if ov.ndim == 1 else _iou3d(a[:, None, :], b[None, :, :], ov)


def iou3d_aligned_oracle(a, b):
    """per-pair 3-D IoU on the CPU oracle's overlap (the iou_fn of heading_sensitivity for the recall inputs)"""
    from oracle import oracle as O

    return iou3d_from_overlap(a, b, O.boxes_aligned_overlap_bev(a, b))


# ------------------------------------------------------------------------------------------------------------------ further inputs
PAIRWISE_SHAPE = (531, 277)      # many 16 x 16 tiles, ragged on both sides
ALIGNED_PAIRS = 10001


@functools.lru_cache(maxsize=None)
def pairwise_inputs():
    """A (531, 7), B (277, 7): B are noisy copies of rows of A, so that a good share of the matrix overlaps, plus the classic
    special pairs on the diagonal (identical, touching, nested, 90 degrees, tiny); a2, b2 (10 001, 7) for the aligned forms."""
    r = np.random.default_rng([SEED, 531, 277])
    na, nb = PAIRWISE_SHAPE
    A = clustered(r, na, spread=25.0)
    B = A[r.permutation(na)[:nb]] + (r.normal(size=(nb, 7)) * NOISE).astype(np.float32)
    B[:, 3:6] = np.maximum(B[:, 3:6], np.float32(0.5))
    B[:5] = A[:5]                                    # identical boxes
    A[5], B[5] = [0, 0, 0, 4, 2, 1, 0.0], [4.0, 0, 0, 4, 2, 1, 0.0]             # touching edge
    A[6], B[6] = [0, 0, 0, 10, 10, 1, 0.2], [0.5, -0.3, 0, 1.5, 0.7, 1, 1.1]    # nested
    A[7], B[7] = [0, 0, 0, 4, 2, 1, 0.0], [0, 0, 0, 4, 2, 1, np.pi / 2]         # 90 degrees
    A[8, 3:5] = 1e-3                                 # tiny
    a2 = clustered(r, ALIGNED_PAIRS)
    b2 = a2 + (r.normal(size=a2.shape) * NOISE).astype(np.float32)
    b2[:, 3:6] = np.maximum(b2[:, 3:6], np.float32(0.5))
    b2[5000:] = clustered(r, ALIGNED_PAIRS - 5000)   # the second half mostly apart
    for x in (A, B, a2, b2):
        x.setflags(write=False)
    return A, B, a2, b2


def cross_pairs(A, B):
    """the candidate pairs (i in A, j in B) of two box sets, j counted in B"""
    p = candidates(np.concatenate([A, B]))
    p = p[(p[:, 0] < A.shape[0]) & (p[:, 1] >= A.shape[0])]
    return np.stack([p[:, 0], p[:, 1] - A.shape[0]], 1)


RECALL_SEED = 4
RECALL_THRESH = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]     # 8, the most fnp_recall_counters takes
RECALL_GT, RECALL_PAD, RECALL_PREDS, RECALL_ROIS = 150, 7, 700, 300
RECALL_ZERO_ROWS = (40, 97)


@functools.lru_cache(maxsize=None)
def recall_inputs(seed=RECALL_SEED):
    """gt (157, 10) with two zero rows in the middle and 7 trailing ones, class label last; preds (700, 7), 300 of them near a
    ground-truth box; rois (300, 7); garbage (7,), a box that WOULD hit if rows past the live count were read."""
    r = np.random.default_rng([SEED, seed, 150])
    G = RECALL_GT
    gt = np.zeros((G + RECALL_PAD, 10), np.float32)
    gt[:G, :7] = clustered(r, G, spread=30.0)
    gt[:G, 7:9] = r.normal(size=(G, 2))
    gt[:G, 9] = r.integers(1, 11, size=G)
    for z in RECALL_ZERO_ROWS:
        gt[z] = 0
    preds = clustered(r, RECALL_PREDS, spread=30.0)
    near = np.arange(300) % G
    preds[:300] = gt[near, :7] + (r.normal(size=(300, 7)) * NOISE * r.uniform(0.2, 6.0, (300, 1))).astype(np.float32)
    preds[:, 3:6] = np.maximum(preds[:, 3:6], np.float32(0.5))
    preds = preds[r.permutation(RECALL_PREDS)]
    rois = preds[:RECALL_ROIS] + np.float32(0.05)
    garbage = gt[149, :7].copy()
    for x in (gt, preds, rois, garbage):
        x.setflags(write=False)
    return gt, preds, rois, garbage


PIB_T, PIB_M, PIB_M_DENSE = 257, 100003, 20011      # 128 + 128 + 1 boxes: three LDS tiles, the last holding one box


@functools.lru_cache(maxsize=None)
def pib_inputs():
    """boxes (257, 7) crowded into +-12 m so that points lie in several boxes, box 256 (alone in the third tile) wide enough to
    hold many points of the earlier tiles too; pts (100 003, 3)"""
    r = np.random.default_rng([SEED, PIB_T, PIB_M])
    boxes = clustered(r, PIB_T, spread=12.0)
    boxes[:, 3:5] = np.minimum(boxes[:, 3:5], np.float32(4.0))
    boxes[256] = [1.0, -2.0, -0.5, 18.0, 16.0, 6.5, 0.3]
    pts = r.uniform(-14, 14, size=(PIB_M, 3)).astype(np.float32)
    pts[:, 2] = r.uniform(-4, 3, size=PIB_M)
    boxes.setflags(write=False)
    pts.setflags(write=False)
    return boxes, pts


def face_grazing(pts, boxes, margin, eps=2e-6):
    """(T, M) pairs whose decision is within float-rounding distance of a face: the only pairs where libm (CPU oracle) and ocml
    (GPU) cos / sin ulps may legitimately flip the flag (the allowance tests/test_gpu_ops.py makes)"""
    out = np.zeros((boxes.shape[0], pts.shape[0]), bool)
    p = pts.astype(np.float64)
    for t, b in enumerate(boxes.astype(np.float64)):
        d = p - b[:3]
        c, s = np.cos(-b[6]), np.sin(-b[6])
        lx, ly = d[:, 0] * c - d[:, 1] * s, d[:, 0] * s + d[:, 1] * c
        scale = np.abs(d[:, :2]).sum(1) + 1.0
        out[t] = (np.abs(np.abs(lx) - (b[3] / 2 + margin)) < eps * scale) | (np.abs(np.abs(ly) - (b[4] / 2 + margin)) < eps * scale)
    return out
