"""CLIP-crop scoring against golden vectors produced by the reference's own
CLIPBoxClassification.forward (tests/golden/make_clipcrop_golden.py): same (box, camera) crop list in the same
order, crops equal through the stand-in encoder's 28x28 average pooling (2e-4), class probabilities (fp16 in
the reference) within 1e-2, re-labelled classes equal wherever the top-2 margin of the recorded mean probabilities
exceeds twice that tolerance.

Below the goldens, the two kernels are held directly to the float64 restatement of tests/ref_clipcrop.py (tied to the
reference's own run on the CPU by tests/test_clipcrop_ref.py): the plan kernel's rect / cam_mask exactly wherever the
restatement's error bounds decide the outcome and inside the admissible ranges elsewhere, at box counts on both sides
of one workgroup and at several; hand-computed exact cases at every comparison of the kernel; and every element of the
sample kernel's output inside its own bound."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_clipcrop as R  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def procedural_images(h, w):
    y, x = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    out = np.empty((6, 3, h, w), np.float32)
    for c in range(6):
        for ch in range(3):
            out[c, ch] = 0.5 + 0.5 * np.sin(np.float32(0.013 * (ch + 1)) * x + np.float32(0.7 * c)) * np.cos(np.float32(0.011) * y + np.float32(0.3 * ch))
    return out


class FakeClip:   # the stand-in encoder of the golden generator
    def __init__(self, dev):
        self.logit_scale = torch.tensor(float(np.log(100.0)), device=dev).half()
        self.P = torch.from_numpy(np.random.default_rng(77).standard_normal((192, 32)).astype(np.float32)).to(dev)
        self.seen = []

    def encode_image(self, images):
        pooled = F.avg_pool2d(images.float(), 28).reshape(images.shape[0], -1)
        self.seen.append(pooled.cpu().numpy())
        return (pooled @ self.P).half()


@pytest.mark.parametrize("seed", [0, 1, 2])   # (2: boxes around the ego and at a camera — corners behind cameras, rectangles clipped at two borders)
def test_clip_crop_scoring_matches_reference_golden(cuda, seed):
    from findnpropagate_amd.dense_heads import CLIPBoxClassification
    g = np.load(os.path.join(GOLD, f"clipcrop_seed{seed}.npz"))
    text = torch.from_numpy(np.random.default_rng(78).standard_normal((10, 32)).astype(np.float32)).half().to(cuda)
    clip = FakeClip(cuda)
    head = CLIPBoxClassification(image_size=[900, 1600], clip_model=clip, text_features=text)
    images = torch.from_numpy(procedural_images(900, 1600)).to(cuda)
    bd = {"batch_size": 1, "camera_imgs": images[None], "img_aug_matrix": torch.from_numpy(g["img_aug"])[None].to(cuda),
          "lidar_aug_matrix": torch.from_numpy(g["lidar_aug"])[None].to(cuda), "lidar2image": torch.from_numpy(g["lidar2image"])[None].to(cuda)}
    pd = [{"pred_boxes": torch.from_numpy(g["boxes"]).to(cuda), "pred_labels": torch.from_numpy(g["orig_labels"]).to(cuda),
           "pred_scores": torch.zeros(g["boxes"].shape[0], device=cuda)}]
    head.forward(bd, pd, keep_crops=True)
    pooled = np.concatenate(clip.seen, 0) if clip.seen else np.zeros((0, 192), np.float32)
    assert pooled.shape == g["pooled"].shape, "same (box, camera) crop list"
    np.testing.assert_allclose(pooled, g["pooled"], rtol=0, atol=2e-4)
    probs = head.crop_infos["logits"].float().numpy()
    np.testing.assert_allclose(probs, g["probs"], rtol=0, atol=1e-2)
    np.testing.assert_allclose(pd[0]["pred_scores"].float().numpy(), g["pred_scores"], rtol=0, atol=1e-2)
    assert np.array_equal(pd[0]["orig_labels"].cpu().numpy(), g["orig_labels"])
    got, want = pd[0]["pred_labels"].cpu().numpy(), g["pred_labels"]
    assert (got == want).mean() >= 0.9 and got.min() >= 1 and got.max() <= 10
    clear = top2_margin(g["probs_mean"]) > 2e-2
    assert clear.sum() >= 3 and np.array_equal(got[clear], want[clear])


def top2_margin(probs_mean):
    t = np.sort(probs_mean.astype(np.float64), axis=1)
    return t[:, -1] - t[:, -2]


def test_clip_crop_scoring_two_augmented_scenes(cuda):
    """clipcrop_aug_b2.npz: the reference's forward on two scenes with their own boxes, lidar_aug_matrix (scene 1: rotation, scaling,
    translation), lidar2image and a non-identity img_aug_matrix per camera (resize, crop shift, a flip, a rotation) at 256 x 704."""
    from findnpropagate_amd.dense_heads import CLIPBoxClassification
    g = np.load(os.path.join(GOLD, "clipcrop_aug_b2.npz"))
    text = torch.from_numpy(np.random.default_rng(78).standard_normal((10, 32)).astype(np.float32)).half().to(cuda)
    clip = FakeClip(cuda)
    head = CLIPBoxClassification(image_size=[256, 704], clip_model=clip, text_features=text)
    one = procedural_images(256, 704)
    images = torch.from_numpy(np.stack([one, one[::-1].copy()], 0)).to(cuda)
    bd = {"batch_size": 2, "camera_imgs": images, "img_aug_matrix": torch.from_numpy(g["img_aug"]).to(cuda),
          "lidar_aug_matrix": torch.from_numpy(g["lidar_aug"]).to(cuda), "lidar2image": torch.from_numpy(g["lidar2image"]).to(cuda)}
    pd = [{"pred_boxes": torch.from_numpy(g[f"boxes{b}"]).to(cuda), "pred_labels": torch.from_numpy(g[f"orig_labels{b}"]).to(cuda),
           "pred_scores": torch.zeros(g[f"boxes{b}"].shape[0], device=cuda)} for b in range(2)]
    at = np.concatenate([[0], np.cumsum(g["crops_per_scene"])])
    for b in range(2):                                   # the crop list itself, per scene: pairs in the reference's order, rectangles equal
        rect, mask = head.plan(bd, pd[b]["pred_boxes"], b)
        rect = rect.cpu().numpy()
        pairs = R.crop_pairs(rect)
        assert np.array_equal(pairs, g["crop_pair"][at[b]:at[b + 1]]), f"scene {b}: same (box, camera) crop list"
        assert np.array_equal(rect[pairs[:, 0], pairs[:, 1], :3].astype(np.int64), g["crop_rect"][at[b]:at[b + 1]].astype(np.int64))
    head.forward(bd, pd, keep_crops=True)
    assert [p.shape[0] for p in clip.seen] == g["crops_per_scene"].tolist()
    np.testing.assert_allclose(np.concatenate(clip.seen, 0), g["pooled"], rtol=0, atol=2e-4)
    np.testing.assert_allclose(head.crop_infos["logits"].float().numpy(), g["probs"], rtol=0, atol=1e-2)
    for b in range(2):
        np.testing.assert_allclose(pd[b]["pred_scores"].float().numpy(), g[f"pred_scores{b}"], rtol=0, atol=1e-2)
        assert np.array_equal(pd[b]["orig_labels"].cpu().numpy(), g[f"orig_labels{b}"])
        got, want = pd[b]["pred_labels"].cpu().numpy(), g[f"pred_labels{b}"]
        clear = top2_margin(g[f"probs_mean{b}"]) > 2e-2
        assert clear.sum() >= 8 and np.array_equal(got[clear], want[clear])
        assert got.min() >= 1 and got.max() <= 10


# ---------------------------------------------------------------------------------------------- plan kernel
def run_plan(cuda, c, n=None):
    """The raw entry point on NaN / 255 pre-filled outputs, with the inverse and translation the module passes."""
    from findnpropagate_amd import lib as _l
    L = _l.load()
    n = len(c["boxes"]) if n is None else n
    aug = torch.from_numpy(c["lidar_aug"])
    rinv, trans = torch.inverse(aug[:3, :3]).contiguous(), aug[:3, 3].contiguous()
    boxes = torch.from_numpy(c["boxes"]).to(cuda).contiguous()
    l2i, iaug = torch.from_numpy(c["l2i"]).to(cuda).contiguous(), torch.from_numpy(c["iaug"]).to(cuda).contiguous()
    rect = torch.full((max(n, 1), 6, 4), float("nan"), dtype=torch.float32, device=cuda)
    mask = torch.full((max(n, 1), 6), 255, dtype=torch.uint8, device=cuda)
    rc = L.fnp_clipcrop_plan(_l.ptr(boxes), n, rinv.data_ptr(), trans.data_ptr(), _l.ptr(l2i), _l.ptr(iaug), c["H"], c["W"], 64,
                             _l.ptr(rect), _l.ptr(mask), _l.stream())
    torch.cuda.synchronize()
    assert rc == 0
    return rect.cpu().numpy(), mask.cpu().numpy(), rinv.numpy(), trans.numpy()


@pytest.mark.parametrize("name", [c[0] for c in R.PLAN_CASES])
def test_plan_random_cases(cuda, name):
    """n * 6 = 6, 252, 258 and 1800 threads: under, just under and just over one 256-thread workgroup, and eight of them; both image
    geometries and lidar augmentations without, with rotation and with scaling (tests/test_clipcrop_ref.py checks on the CPU that
    each case decides >= 95 % of its candidate pairs and contains crops and too-small crops)."""
    c = R.plan_case(name)
    rect, mask, rinv, trans = run_plan(cuda, c)
    rect2, mask2, _, _ = run_plan(cuda, c)
    assert rect.tobytes() == rect2.tobytes() and mask.tobytes() == mask2.tobytes(), "two runs, same bits"
    assert np.isfinite(rect).all() and (mask <= 1).all(), "every element written"
    args = (c["boxes"], rinv, trans, c["l2i"], c["iaug"])
    p = R.plan(*args, c["H"], c["W"])
    bad = R.check_plan(p, rect, mask)
    # The kernel does not store its projection, so the device's own |f32 - f64| / bound cannot be formed; through rect a decided pair
    # says only that the device's extreme corners fell in the restatement's pixel.  Printed instead: the same chain replayed in f32 on the host.
    vals = R.project(*args)
    keep = (vals[3][0] - vals[3][1] > 1e-5) & (vals[3][0] + vals[3][1] < 1e5)
    may = p["mask_hi"]
    print(f"RATIO plan {name}: decided {(p['decided'] & may).sum() / may.sum():.4f} of {int(may.sum())} candidate pairs, device equals the restatement on "
          f"{int(p['decided'].sum()) - sum(b.startswith('decided') for b in bad)} of {int(p['decided'].sum())} decided pairs, crops {int((rect[..., 3] > 0).sum())}, "
          f"host f32 replay / bound {R.worst_ratio(vals[:3], R.replay_f32(*args), keep):.3f}")
    assert not bad, bad[:5]


def test_plan_exact_edge_cases(cuda):
    """Hand-computed cases on which every f32 operation is exact (dyadic pinhole, yaw 0): a corner at column 0, W - 1, W, W + 1, in
    (-1, 0) and at -1; rz = 2^-7 and 2^-6 around 0.01; side 63 and 64; behind the camera; across the camera plane; all corners off
    the image around it; an img_aug with a depth term.  Expected values: ref_clipcrop.edge_cases (checked on the CPU)."""
    wrong = []
    for name, c in R.edge_cases().items():
        rect, mask, _, _ = run_plan(cuda, c)
        m, r = c["expect"]
        if not (np.all(mask == m) and np.all(rect == np.array(r, np.float32))):
            wrong.append((name, mask[0].tolist(), rect[0, 0].tolist(), m, r))
    assert not wrong, wrong


def test_plan_no_boxes(cuda):
    c = dict(R.edge_cases()["inside"])
    rect, mask, _, _ = run_plan(cuda, c, n=0)
    assert np.isnan(rect).all() and (mask == 255).all()


# ---------------------------------------------------------------------------------------------- sample kernel
_IMAGES = {}


def sample_images(kind, C, dtype):
    """(6, C, H, W) in the stored dtype, and its SampleRef; made once per kind."""
    key = (kind, C, dtype)
    if key not in _IMAGES:
        rng = np.random.default_rng(4321)
        if kind == "noise_120x200":
            img = rng.uniform(0, 1, (6, C, 120, 200)).astype(np.float32)
        else:
            H, W = (256, 704) if kind == "256x704" else (900, 1600)
            base = procedural_images(H, W)
            img = base[:, [ch % 3 for ch in range(C)]] * np.float32(0.9) + rng.uniform(0, 0.1, (6, C, H, W)).astype(np.float32)
        img = img.astype(dtype)
        _IMAGES[key] = (img, R.SampleRef(img))
    return _IMAGES[key]


def sample_pairs(M, rng):
    """Few: all six cameras, not ascending, one pair twice.  Many: random (box, camera), repeats included."""
    if M == 1:
        return np.array([[1, 5]], np.int32)
    if M == 8:
        return np.array([[0, 2], [1, 5], [2, 0], [3, 1], [4, 3], [0, 4], [1, 5], [0, 0]], np.int32)
    return np.stack([rng.integers(0, 5, M), rng.integers(0, 6, M)], 1).astype(np.int32)


def check_crops(got, ref, rects, pairs, unit, f16):
    worst, where = 0.0, None
    assert np.isfinite(got).all(), "every element written"
    seen = {}
    for m, (b, c) in enumerate(pairs.tolist()):
        if (b, c) not in seen:
            seen[(b, c)] = ref.crop(c, *rects[b, c, :3], unit, f16_out=f16)
        val, bound = seen[(b, c)]
        err = np.abs(got[m].astype(np.float64) - val)
        assert np.all(err[bound == 0] == 0), (m, b, c, "exact zeros")
        r = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        if r > worst:
            worst, where = r, (m, b, c)
    return worst, where


SAMPLE_CASES = [  # image, C, dtype, S, M
    ("noise_120x200", 3, np.float32, 224, 8),
    ("noise_120x200", 3, np.float16, 224, 8),
    ("noise_120x200", 1, np.float16, 13, 300),
    ("256x704", 4, np.float32, 8, 1),
    ("256x704", 4, np.float16, 13, 300),
    ("256x704", 1, np.float32, 1, 300),
    ("900x1600", 3, np.float32, 224, 8),
    ("900x1600", 3, np.float16, 224, 8),
    ("900x1600", 3, np.float32, 13, 300),
]


@pytest.mark.parametrize("kind,C,dtype,S,M", SAMPLE_CASES, ids=[f"{k}-C{C}-{np.dtype(d).name}-S{S}-M{M}" for k, C, d, S, M in SAMPLE_CASES])
def test_sample_every_element_inside_its_bound(cuda, rng, kind, C, dtype, S, M):
    """fnp_clipcrop_sample on a NaN pre-filled output against the f64 bilinear restatement: S a multiple of the 8 rows of a workgroup,
    not one, and 1; one pair and 300 in grid.y; rectangles inside, overhanging, larger than the image, starting at x = W, ending at
    the far corner; f16 images upcast exactly, positions kept in f32."""
    from findnpropagate_amd import lib as _l
    L = _l.load()
    img, ref = sample_images(kind, C, dtype)
    H, W = img.shape[2:]
    rects = np.repeat(R.sample_rects(H, W)[:, None, :], 6, 1).copy()
    unit = R.unit_table(S) if S in (224, 1, 8) else np.sort(rng.uniform(0, 1, S)).astype(np.float32)     # any ascending table in [0, 1]
    pairs = sample_pairs(M, rng)
    t_img, t_rect, t_pairs, t_unit = (torch.from_numpy(a).to(cuda).contiguous() for a in (img, rects, pairs, unit))
    out = torch.full((M, C, S, S), float("nan"), dtype=t_img.dtype, device=cuda)
    rc = L.fnp_clipcrop_sample(_l.ptr(t_img), _l.dtype_code(t_img), C, H, W, _l.ptr(t_rect), _l.ptr(t_pairs), M, _l.ptr(t_unit), S, _l.ptr(out),
                               _l.stream())
    torch.cuda.synchronize()
    assert rc == 0
    worst, where = check_crops(out.cpu().numpy(), ref, rects, pairs, unit, dtype == np.float16)
    print(f"RATIO sample {kind} C={C} {np.dtype(dtype).name} S={S} M={M}: worst |device - f64| / bound {worst:.3f} at (pair, box, camera) {where}")
    assert worst <= 1.0


@pytest.mark.parametrize("kind,dtype", [("noise_120x200", np.float32), ("noise_120x200", np.float16), ("900x1600", np.float32)])
def test_head_sample_inside_its_bound(cuda, rng, kind, dtype):
    """The module's own sample(): its 224-entry table from torch's affine_grid, its allocation and argument order."""
    from findnpropagate_amd.dense_heads import CLIPBoxClassification
    img, ref = sample_images(kind, 3, dtype)
    H, W = img.shape[2:]
    head = CLIPBoxClassification(image_size=[H, W], clip_model=object(), text_features=torch.ones(10, 3))
    rects = np.repeat(R.sample_rects(H, W)[:, None, :], 6, 1).copy()
    pairs = sample_pairs(8, rng)
    got = head.sample(torch.from_numpy(img).to(cuda), torch.from_numpy(rects).to(cuda), torch.from_numpy(pairs).to(cuda))
    assert got.shape == (8, 3, 224, 224) and got.dtype == (torch.float32 if dtype == np.float32 else torch.float16)
    worst, where = check_crops(got.cpu().numpy(), ref, rects, pairs, head._unit.numpy(), dtype == np.float16)
    print(f"RATIO head.sample {kind} {np.dtype(dtype).name}: worst |device - f64| / bound {worst:.3f} at (pair, box, camera) {where}")
    assert worst <= 1.0


def test_sample_argument_errors_launch_nothing(cuda):
    """bf16 images, 65,536 pairs (grid.y stops at 65,535) and out_size 0 are refused before any launch: FNP_ERR_ARG, output untouched."""
    from findnpropagate_amd import lib as _l
    L = _l.load()
    img = torch.zeros((6, 1, 16, 16), device=cuda)
    rect = torch.tensor([0., 0., 64., 1.], device=cuda).repeat(1, 6, 1).contiguous()
    pairs = torch.zeros((4, 2), dtype=torch.int32, device=cuda)
    unit = torch.linspace(0, 1, 8, device=cuda)
    out = torch.full((4, 1, 8, 8), float("nan"), device=cuda)

    def call(image, num_pairs, S):
        rc = L.fnp_clipcrop_sample(_l.ptr(image), _l.dtype_code(image), 1, 16, 16, _l.ptr(rect), _l.ptr(pairs), num_pairs, _l.ptr(unit), S, _l.ptr(out),
                                   _l.stream())
        torch.cuda.synchronize()
        return rc
    assert call(img.to(torch.bfloat16), 4, 8) == -1
    assert call(img, 65536, 8) == -1
    assert call(img, 4, 0) == -1
    assert torch.isnan(out).all()
    assert call(img, 4, 8) == 0 and torch.isfinite(out).all()      # the same call with admissible arguments does write


def test_crop_equals_grid_sample(cuda, rng):
    """fnp_clipcrop_sample against torch's own F.grid_sample on the grid the reference builds (:313-334)."""
    from findnpropagate_amd.dense_heads import CLIPBoxClassification

    class Enc:
        logit_scale = torch.zeros((), device="cuda")

        def encode_image(self, x):
            return x.mean(dim=(2, 3))
    head = CLIPBoxClassification(image_size=[120, 200], clip_model=Enc(), text_features=torch.ones(10, 3))
    images = torch.from_numpy(rng.uniform(0, 1, (6, 3, 120, 200)).astype(np.float32)).to(cuda)
    rect = torch.zeros((3, 6, 4), device=cuda)
    rect[0, 2] = torch.tensor([10., 20., 64., 1.])
    rect[1, 5] = torch.tensor([150., 0., 90., 1.])          # runs off the right and bottom edges: zero padding
    rect[2, 0] = torch.tensor([0., 60., 70., 1.])
    pairs = torch.tensor([[0, 2], [1, 5], [2, 0]], dtype=torch.int32, device=cuda)
    for dt in (torch.float32, torch.float16):
        got = head.sample(images.to(dt), rect, pairs)
        unit = head._unit.to(cuda)
        for m, (b, c) in enumerate(pairs.tolist()):
            x1, y1, side, _ = rect[b, c].tolist()
            gx, gy = unit[None, :].expand(224, 224) * side + x1, unit[:, None].expand(224, 224) * side + y1
            grid = torch.stack([(gx / 200) * 2 - 1, (gy / 120) * 2 - 1], -1)[None]
            # (torch's f16 grid_sample also rounds the sampling positions to f16; the kernel keeps them in f32,
            #  so both dtypes are held against the f32 result)
            want = F.grid_sample(images[[c]], grid, align_corners=False)
            tol = 1e-4 if dt == torch.float32 else 2e-3   # 1e-4: the fp32 bar of BASELINE.json (white-noise image, rounding of the sampling positions)
            assert (got[m].float() - want[0].float()).abs().max() <= tol
