"""The box operators (csrc/iou3d_nms.hip, csrc/points_in_boxes.hip) at the sizes where their kernels change form, each kernel
on its own: the suppression mask is read back from a workspace the test owns, so the sweep is held to tests/ref_box.host_sweep
over the DEVICE's mask (exact) and the mask to the axis-aligned restatement (exact), to the CPU oracle outside the measured BAND
and, where oracle/_ref travelled, to the reference's own kernels on this GPU (exact).  Inputs and checkers are those of
tests/ref_box.py; tests/test_ref_box.py shows on the CPU that they can fail.  One FORM line per case."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ref_box as R

pytestmark = pytest.mark.gpu
REF_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref")
SENTINEL = -1     # all-ones words / keep slots: whatever the kernels do not write stays so


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _dev(a, cuda):
    return torch.tensor(np.ascontiguousarray(a), device=cuda)


def _ref_iou3d():
    """the reference's iou3d kernels, None where oracle/_ref was not built — but a build that brought the point-in-box library
    and not this one is broken, not absent (as test_reference_point_in_box_kernel_is_the_checker_... holds the other way round)"""
    from oracle import ref_loader

    lib = ref_loader.iou3d_gpu_lib()
    if lib is None:
        assert not os.path.exists(os.path.join(REF_DIR, "libref_pib_gpu.so")), \
            "oracle/_ref/libref_iou3d_gpu.so missing although libref_pib_gpu.so is there: run `make -C oracle ref` where the reference is"
    return lib


def _ref_mask(ref, d_boxes, n, thresh, rotated):
    mask = torch.zeros((n * R.words(n),), dtype=torch.int64, device=d_boxes.device)
    (ref.ref_nms_mask if rotated else ref.ref_nms_normal_mask)(_p(d_boxes), _p(mask), n, ctypes.c_float(thresh))
    torch.cuda.synchronize()
    return mask.cpu().numpy().view(np.uint64).reshape(n, R.words(n))


def _nms(cuda, boxes, thresh, rotated):
    """fnp_nms_rotated / fnp_nms_normal through the C ABI on a workspace with 64 spare rows -> (mask (n, cb) uint64, keep, device
    boxes); holds what both flavours owe: rows past n of the workspace stay 0, keep past num_keep stays untouched"""
    from findnpropagate_amd import lib as _l

    L = _l.load()
    n, cb = boxes.shape[0], R.words(boxes.shape[0])
    assert int(L.fnp_nms_workspace_bytes(n)) == n * cb * 8
    d = _dev(boxes, cuda)
    ws = torch.full(((n + 64) * cb,), SENTINEL, dtype=torch.int64, device=cuda)
    ws[n * cb:] = 0
    keep = torch.full((n + 64,), SENTINEL, dtype=torch.int64, device=cuda)
    num = torch.full((1,), -7, dtype=torch.int32, device=cuda)
    rc = (L.fnp_nms_rotated if rotated else L.fnp_nms_normal)(_l.ptr(d), n, float(thresh), _l.ptr(ws), _l.ptr(keep), _l.ptr(num), _l.stream())
    assert rc == 0
    torch.cuda.synchronize()
    w = ws.cpu().numpy().view(np.uint64)
    assert not w[n * cb:].any(), "rows past n were written"
    k, m = keep.cpu().numpy(), int(num.item())
    assert 0 <= m <= n and (k[m:] == SENTINEL).all(), "keep past num_keep was written"
    return R.decode_ws(w, n), k[:m], d


@pytest.mark.parametrize("rotated", [True, False], ids=["rotated", "normal"])
@pytest.mark.parametrize("n,thresh", R.NMS_CASES)
def test_nms_mask_and_sweep_at_scale(cuda, oracle, n, thresh, rotated):
    case = (R.rotated_case if rotated else R.normal_case)(n, thresh)
    mask, keep, d = _nms(cuda, case["boxes"], thresh, rotated)
    sweep_ok = np.array_equal(keep, R.host_sweep(mask, n))                      # 1. the sweep alone, over the device's own mask
    found = (R.check_mask_rotated if rotated else R.check_mask_normal)(mask, case)   # 2. the mask alone
    over = int(case["over"].sum()) if rotated else int(R.get_bits(case["mask"], case["pairs"]).sum())
    und = int(case["undecided"].sum()) if rotated else 0
    ref = _ref_iou3d()
    ref_words = ref_keep_ok = None
    if ref is not None:                                                         # 3. the reference's kernel on this GPU
        rm = _ref_mask(ref, d, n, thresh, rotated)
        up = R.upper_words(n)                                                   # (it fills the tiles left of the diagonal too)
        ref_words = int(np.count_nonzero((mask != rm) & up))
        ref_keep_ok = np.array_equal(keep, R.host_sweep(rm, n))
    checker = "reference kernel + oracle" if ref is not None else "oracle"
    print(f"FORM nms {'rotated' if rotated else 'normal'} n {n} words {R.words(n)} thresh {thresh} candidates {len(case['pairs'])} "
          f"over {over} undecided {und} ({und / max(over, 1):.4%}) kept {len(keep)} mask {found} "
          f"words differing from the reference kernel {ref_words} checker {checker}")
    assert sweep_ok, "the sweep's keep list differs from host_sweep over the device's own mask"
    assert found["non_candidate"] == 0 and found["past_n"] == 0
    if rotated:
        assert found["decided_wrong"] == 0, "a bit outside the band differs from the oracle"
        assert und <= R.UNDECIDED_SHARE_CAP * over
    else:
        assert found["words_differ"] == 0, "the axis-aligned mask differs from its float32 restatement"
    if ref is not None:
        assert ref_words == 0, "the mask differs from the reference kernel's at or right of the diagonal"
        assert ref_keep_ok, "keep list differs from host_sweep over the reference kernel's mask"
    if und == 0:                                                                # 4. the oracle's whole NMS
        assert np.array_equal(keep, oracle.nms(case["boxes"], thresh, rotated))
    if thresh == 1.0:
        assert len(keep) == n


@pytest.mark.parametrize("rotated", [True, False], ids=["rotated", "normal"])
def test_batched_nms_at_scale(cuda, rotated):
    """fnp_nms_batched: list z's mask starts at z * cap * ceil(cap / 64) words with the row stride of its OWN count"""
    from findnpropagate_amd import lib as _l

    L = _l.load()
    cap, counts, thresh = 4800, [4800, 4161, 4096, 65, 0], 0.1
    slab = cap * R.words(cap)
    boxes = np.full((len(counts), cap, 7), 1.0e6, np.float32)        # rows past a list's count must never be read as boxes
    for z, c in enumerate(counts):
        if c:
            boxes[z, :c] = R.make_boxes(c)
    d, d_counts = _dev(boxes, cuda), torch.tensor(counts, dtype=torch.int32, device=cuda)
    assert int(L.fnp_nms_batched_workspace_bytes(len(counts), cap)) == len(counts) * slab * 8
    ws = torch.full((len(counts) * slab,), SENTINEL, dtype=torch.int64, device=cuda)
    keep = torch.full((len(counts), cap), SENTINEL, dtype=torch.int64, device=cuda)
    num = torch.full((len(counts),), -7, dtype=torch.int32, device=cuda)
    rc = L.fnp_nms_batched(_l.ptr(d), _l.ptr(d_counts), len(counts), cap, thresh, int(rotated), _l.ptr(ws), _l.ptr(keep), _l.ptr(num), _l.stream())
    assert rc == 0
    torch.cuda.synchronize()
    w, keep, num = ws.cpu().numpy().view(np.uint64), keep.cpu().numpy(), num.cpu().numpy()
    masks = R.decode_ws_batched(w, cap, counts)
    for z, c in enumerate(counts):
        m = int(num[z])
        used = c * R.words(c)
        print(f"FORM nms batched {'rotated' if rotated else 'normal'} list {z} count {c} words {R.words(c)} kept {m}")
        assert (keep[z, m:] == SENTINEL).all(), "keep past num_keep was written"
        assert (w[z * slab + used: (z + 1) * slab] == ~np.uint64(0)).all(), "the slab was written past the list's own mask"
        if c == 0:
            assert m == 0
            continue
        m1, k1, _ = _nms(cuda, R.make_boxes(c), thresh, rotated)
        assert np.array_equal(masks[z], m1), "mask slice differs from the single-list call"
        assert m == len(k1) and np.array_equal(keep[z, :m], k1)
        assert np.array_equal(keep[z, :m], R.host_sweep(masks[z], c))
    assert 0 < num[0] < 4800 and 0 < num[3] <= 65


def test_pairwise_kernels_at_scale(cuda, oracle):
    from findnpropagate_amd import lib as _l

    L = _l.load()
    A, B, a2, b2 = R.pairwise_inputs()
    (na, nb), n2 = R.PAIRWISE_SHAPE, R.ALIGNED_PAIRS
    a, b, da2, db2 = (_dev(x, cuda) for x in (A, B, a2, b2))
    nan = lambda *shape: torch.full(shape, float("nan"), device=cuda)
    ov, iou, i3, al, al3, al2, al23 = nan(na, nb), nan(na, nb), nan(na, nb), nan(nb), nan(nb), nan(n2), nan(n2)
    s = _l.stream()
    a_head = a[:nb].contiguous()
    for rc in (L.fnp_boxes_overlap_bev(_l.ptr(a), na, _l.ptr(b), nb, _l.ptr(ov), s),
               L.fnp_boxes_iou_bev(_l.ptr(a), na, _l.ptr(b), nb, _l.ptr(iou), s),
               L.fnp_boxes_iou3d(_l.ptr(a), na, _l.ptr(b), nb, _l.ptr(i3), s),
               L.fnp_boxes_aligned_overlap_bev(_l.ptr(a_head), _l.ptr(b), nb, _l.ptr(al), s),
               L.fnp_boxes_aligned_iou3d(_l.ptr(a_head), _l.ptr(b), nb, _l.ptr(al3), s),
               L.fnp_boxes_aligned_overlap_bev(_l.ptr(da2), _l.ptr(db2), n2, _l.ptr(al2), s),
               L.fnp_boxes_aligned_iou3d(_l.ptr(da2), _l.ptr(db2), n2, _l.ptr(al23), s)):
        assert rc == 0
    torch.cuda.synchronize()
    # the aligned forms are the diagonal of the pairwise ones: same device function, same bits
    assert torch.equal(al, torch.diagonal(ov)[:nb]) and torch.equal(al3, torch.diagonal(i3)[:nb])
    g = {k: t.cpu().numpy() for k, t in dict(ov=ov, iou=iou, i3=i3, al2=al2, al23=al23).items()}
    assert not any(np.isnan(v).any() for v in g.values())
    # the 3-D IoU is float32 arithmetic on the BEV overlap: bit for bit from the device's own overlap
    assert np.array_equal(g["i3"], R.iou3d_from_overlap(A, B, g["ov"]))
    assert np.array_equal(g["al23"], R.iou3d_from_overlap(a2, b2, g["al2"]))
    ref = _ref_iou3d()
    if ref is not None:
        r_ov, r_iou, r_al = torch.zeros_like(ov), torch.zeros_like(iou), torch.zeros_like(al2)
        ref.ref_boxes_overlap(na, _p(a), nb, _p(b), _p(r_ov))
        ref.ref_boxes_iou_bev(na, _p(a), nb, _p(b), _p(r_iou))
        ref.ref_boxes_aligned_overlap(n2, _p(da2), _p(db2), _p(r_al))
        torch.cuda.synchronize()
        for name, got, want in (("overlap", ov, r_ov), ("iou_bev", iou, r_iou), ("aligned overlap", al2, r_al)):
            assert torch.equal(got, want), f"{name}: max diff {(got - want).abs().max().item()} from the reference's kernel"
    w_ov, w_iou, w_i3, w_al = oracle.boxes_overlap_bev(A, B), oracle.boxes_iou_bev(A, B), oracle.boxes_iou3d(A, B), oracle.boxes_aligned_overlap_bev(a2, b2)
    print(f"FORM pairwise {na} x {nb} overlapping {(w_ov > 0).sum()} aligned {n2} overlapping {(w_al > 0).sum()} max |diff| to the oracle: "
          f"overlap {np.abs(g['ov'] - w_ov).max():.2e} iou_bev {np.abs(g['iou'] - w_iou).max():.2e} iou3d {np.abs(g['i3'] - w_i3).max():.2e} "
          f"aligned overlap {np.abs(g['al2'] - w_al).max():.2e} checker {'reference kernel + oracle' if ref is not None else 'oracle'}")
    np.testing.assert_allclose(g["ov"], w_ov, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(g["al2"], w_al, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(g["iou"], w_iou, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(g["i3"], w_i3, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(g["al23"], R.iou3d_from_overlap(a2, b2, w_al), rtol=1e-4, atol=1e-5)


def test_recall_counters_at_scale(cuda, oracle):
    """150 ground-truth rows (10 tiles of 16, the last ragged) with zero rows in the middle, 700 predictions (44 tiles) as the
    strided body of a record with garbage past the live count, 300 rois, 8 thresholds, three frames accumulated"""
    from findnpropagate_amd.detectors import Detector3DTemplate

    gt, preds, rois, garbage = R.recall_inputs()
    thr = R.RECALL_THRESH
    rec = torch.zeros((1 + R.RECALL_PREDS + 12, 9), device=cuda)
    rec[1:1 + R.RECALL_PREDS, :7] = _dev(preds, cuda)
    rec[1:, 7] = 0.5
    rec[1:, 8] = 1.0
    rec[1 + R.RECALL_PREDS:, :7] = _dev(garbage, cuda)       # a sure hit, were rows past the live count read
    rec[0, 0] = float(R.RECALL_PREDS)
    vec = torch.zeros((5 + 6 * len(thr),), dtype=torch.int64, device=cuda)
    for _ in range(3):
        Detector3DTemplate.recall_counter_vector(rec[1:], _dev(gt, cuda), thr, rois=_dev(rois, cuda), pred_count=rec[0, 0:1], out=vec)
    want = {}
    for _ in range(3):
        want = oracle.generate_recall_record(preds, want, gt, rois, thr)
    keys = ["gt", "num_3known", "num_6known", "num_4unknown", "num_7unknown"]
    for t in thr:
        keys += [stem % str(t) for stem in ("roi_%s", "rcnn_%s", "rcnn_3known_%s", "rcnn_6known_%s", "rcnn_4unknown_%s", "rcnn_7unknown_%s")]
    got = dict(zip(keys, vec.cpu().tolist()))
    print(f"FORM recall gt {want['gt']} rcnn {[want['rcnn_%s' % t] for t in thr]} roi {[want['roi_%s' % t] for t in thr]} equal {got == want}")
    assert got == want
    assert want["gt"] == 3 * R.RECALL_GT and want["rcnn_0.1"] > want["rcnn_0.8"] > 0 and want["roi_0.5"] > 0


def test_points_in_boxes_at_scale(cuda, oracle):
    """T = 257 boxes = 128 + 128 + 1 LDS tiles, M = 100 003 points (391 workgroups, the last ragged)"""
    import ref_pib
    from findnpropagate_amd.roiaware_pool3d import roiaware_pool3d_utils as U

    boxes, pts = R.pib_inputs()
    d_boxes, d_pts = _dev(boxes, cuda), _dev(pts, cuda)
    got = U.points_in_boxes_gpu(d_pts[None], d_boxes[None])[0].cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (R.PIB_M,)
    ref = ref_pib.lib_or_none()
    if ref is not None:      # the reference's own kernel on this GPU: no allowance
        assert np.array_equal(got, ref_pib.points_in_boxes(ref, d_boxes[None], d_pts[None])[0].cpu().numpy())
    else:                    # the libm oracle: only face-grazing points may differ
        diff = got != oracle.points_in_boxes(pts[None], boxes[None])[0]
        assert not (diff & ~R.face_grazing(pts, boxes, 1e-5).any(0)).any() and diff.sum() <= 2
    # a point's FIRST box counts, also when a later tile holds the point too
    d_in3 = U.points_in_boxes_gpu(d_pts[None], d_boxes[None, 256:])[0].cpu().numpy() >= 0
    d_in2 = U.points_in_boxes_gpu(d_pts[None], d_boxes[None, 128:256].contiguous())[0].cpu().numpy() >= 0
    n12, n23, n3 = ((got >= 0) & (got < 128) & d_in2).sum(), ((got >= 128) & (got < 256) & d_in3).sum(), (got == 256).sum()
    assert min(n12, n23, n3) > 100 and not (d_in3 & (got < 0)).any() and not (d_in2 & ((got < 0) | (got > 255))).any()
    cnt = U.points_in_boxes_count(d_pts, d_boxes).cpu().numpy()
    loop = [int((U.points_in_boxes_gpu(d_pts[None], d_boxes[None, t:t + 1].contiguous()) >= 0).sum()) for t in range(R.PIB_T)]
    assert cnt.tolist() == loop and cnt.sum() > R.PIB_M // 4
    m = R.PIB_M_DENSE
    dense = U.points_in_boxes_cpu(d_pts[:m], d_boxes).cpu().numpy()
    flags = int((dense != oracle.points_in_boxes_dense(pts[:m], boxes)).sum())
    print(f"FORM points-in-boxes T {R.PIB_T} M {R.PIB_M} first box in tile 1 / 2 / 3 with a later tile holding the point too "
          f"{n12} / {n23} / {n3} inside any {int((got >= 0).sum())} dense flags differing from the oracle {flags} "
          f"checker {'reference kernel' if ref is not None else 'oracle'}")
    assert dense.shape == (R.PIB_T, m) and flags <= 1
