"""fnp_tf_assign_match (csrc/tfassign.hip) against scipy's linear_sum_assignment on the same f32 matrices: exact, on random,
tie-heavy and duplicated-column costs, at the sizes where the kernel changes route (the transpose at Mvalid < K, a lane's
second column at 65, the square matrix) and with several scenes of different sizes in one launch.  Second half: the cost
and target kernels and QueryTargets end to end against the fixture recorded from the reference's own get_targets
(tests/golden/assign_golden.npz), exact where the outputs are discrete, inside the derived bounds of tests/ref_assign.py elsewhere."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import ref_assign as R
from findnpropagate_amd.dense_heads.transfusion_assign import hungarian_match

pytestmark = pytest.mark.gpu

GPU_FORMS = ("normal", "int", "dup", "01")


def _scipy_assigned(cost, nv, vmap):
    K = cost.shape[0]
    want = np.full(K, -1, np.int32)
    if nv:
        r, c = linear_sum_assignment(cost[:, :nv])
        want[r] = vmap[c]
    return want


def _scenes(seed, K, nvs, forms, Mcap):
    """One batch: scene s is a K x nvs[s] matrix of forms[s] in the leading columns of a NaN-filled (K, Mcap) plane (the
    kernel must not look behind num_valid), an ascending compact -> original map, and an IoU plane that leaves [0, 1]."""
    rng = np.random.default_rng(seed)
    B = len(nvs)
    cost = np.full((B, K, Mcap), np.nan, np.float32)
    vmap = np.full((B, Mcap), -7, np.int32)
    for s, (nv, form) in enumerate(zip(nvs, forms)):
        if nv:
            cost[s, :, :nv] = R.matrix(rng, K, nv, form)
            vmap[s, :nv] = np.sort(rng.choice(2 * Mcap, nv, replace=False))
    iou = rng.uniform(-0.25, 1.25, (B, K, Mcap)).astype(np.float32)
    return cost, np.asarray(nvs, np.int32), vmap, iou


def _run(cuda, cost, nv, vmap, iou):
    a, m = hungarian_match(torch.from_numpy(cost).to(cuda), torch.from_numpy(nv).to(cuda), torch.from_numpy(vmap).to(cuda),
                           torch.from_numpy(iou).to(cuda))
    return a.cpu().numpy(), m.cpu().numpy()


def _check(cost, nv, vmap, iou, got_a, got_iou):
    for s in range(cost.shape[0]):
        want = _scipy_assigned(cost[s], int(nv[s]), vmap[s])
        assert np.array_equal(got_a[s], want), (s, int(nv[s]), np.flatnonzero(got_a[s] != want)[:8].tolist())
        hit = np.flatnonzero(want >= 0)
        col = np.searchsorted(vmap[s, :int(nv[s])], want[hit])
        want_iou = np.zeros(cost.shape[1], np.float32)
        want_iou[hit] = np.clip(iou[s, hit, col], 0.0, 1.0)
        assert np.array_equal(got_iou[s], want_iou)
        assert len(hit) == min(cost.shape[1], int(nv[s]))


SHAPES = [(200, nv) for nv in (0, 1, 2, 37, 63, 64, 65, 199, 200, 201, 260)] + [(K, 40) for K in (1, 64, 65, 256, 257, 300)]


@pytest.mark.parametrize("K,nv", SHAPES)
def test_match_equals_scipy(cuda, K, nv):
    """Every form at this shape, one scene each, in one launch."""
    cost, nvs, vmap, iou = _scenes(1000 * K + nv, K, [nv] * len(GPU_FORMS), GPU_FORMS, Mcap=nv + 3)
    got_a, got_iou = _run(cuda, cost, nvs, vmap, iou)
    _check(cost, nvs, vmap, iou, got_a, got_iou)


def test_scenes_of_different_sizes_and_alone(cuda):
    """Four scenes with different num_valid in one call, both orientations among them; each also equals its own result when
    it is run alone, and a second run gives the same bits."""
    nvs, forms = [5, 0, 48, 37], ["int", "normal", "dup", "normal"]
    cost, nv, vmap, iou = _scenes(5, 40, nvs, forms, Mcap=48)        # K = 40: 5 and 37 transpose, 48 does not
    got_a, got_iou = _run(cuda, cost, nv, vmap, iou)
    _check(cost, nv, vmap, iou, got_a, got_iou)
    again_a, again_iou = _run(cuda, cost, nv, vmap, iou)
    assert np.array_equal(again_a, got_a) and np.array_equal(again_iou.view(np.int32), got_iou.view(np.int32))
    for s in range(len(nvs)):
        a, m = _run(cuda, cost[s:s + 1], nv[s:s + 1], vmap[s:s + 1], iou[s:s + 1])
        assert np.array_equal(a[0], got_a[s]) and np.array_equal(m[0], got_iou[s])


def test_fixed_tie_cases(cuda):
    """The two named matrices of the CPU solver tests: 200 x 37 with 7 duplicated columns, 200 x 60 of integers 0..3."""
    fixed = R.fixed_cases()
    for name in ("200x37 dup7", "200x60 int"):
        m = fixed[name]
        K, nv = m.shape
        cost = m[None].copy()
        a = hungarian_match(torch.from_numpy(cost).to(cuda), torch.tensor([nv], dtype=torch.int32, device=cuda)).cpu().numpy()
        assert np.array_equal(a[0], _scipy_assigned(m, nv, np.arange(nv, dtype=np.int32))), name


def test_no_boxes_and_num_valid_clamped(cuda):
    """Mcap = 0 and num_valid = 0 give no match; a num_valid above Mcap is read as Mcap, a negative one as 0."""
    empty = hungarian_match(torch.empty((2, 7, 0), device=cuda), torch.zeros(2, dtype=torch.int32, device=cuda))
    assert (empty.cpu().numpy() == -1).all() and empty.shape == (2, 7)
    rng = np.random.default_rng(3)
    m = R.matrix(rng, 9, 6, "normal")
    cost = torch.from_numpy(np.stack([m, m])).to(cuda)
    a = hungarian_match(cost, torch.tensor([600, -4], dtype=torch.int32, device=cuda)).cpu().numpy()
    assert np.array_equal(a[0], _scipy_assigned(m, 6, np.arange(6, dtype=np.int32)))
    assert (a[1] == -1).all()


def test_match_reads_nothing_back(cuda):
    """The call runs with host synchronisation forbidden: inputs and outputs stay on the device."""
    cost, nv, vmap, iou = _scenes(11, 200, [37, 12], ["normal", "int"], Mcap=48)
    args = [torch.from_numpy(x).to(cuda) for x in (cost, nv, vmap, iou)]
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a, m = hungarian_match(*args)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    _check(cost, nv, vmap, iou, a.cpu().numpy(), m.cpu().numpy())


# ---- cost, targets: the fixture of the reference's get_targets (tests/golden/assign_golden.npz) ---------------------------------

def _query_targets(name):
    from findnpropagate_amd.dense_heads.transfusion_assign import QueryTargets
    cfg = R.CASES[name]
    tcfg = dict(FEATURE_MAP_STRIDE=R.STRIDE, HUNGARIAN_ASSIGNER=R.ASSIGNER)
    return QueryTargets(tcfg, R.RANGE, R.VOXEL, cfg["C"], code_size=cfg["code"], unknown_labels=cfg["unknown_labels"])


_runs = {}


def _fixture_run(cuda, name):
    """the fixture's inputs through QueryTargets once per case, shared by the tests below (host copies; nothing is modified)"""
    if name not in _runs:
        g = R.golden()
        preds = {h: g[f"{name}_pred_{h}"] for h, _ in R.HEAD_DIMS if f"{name}_pred_{h}" in g}
        gt = g[f"{name}_gt_boxes"]
        out = _query_targets(name)({h: torch.from_numpy(v).to(cuda) for h, v in preds.items()}, torch.from_numpy(gt).to(cuda),
                                   return_debug=True)
        _runs[name] = (g, preds, gt, {k: v.cpu().numpy() for k, v in out.items()}, out)
    return _runs[name]


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_cost_kernel(cuda, name):
    g, preds, gt, out, dev = _fixture_run(cuda, name)
    cfg = R.CASES[name]
    w_iou = np.float32(R.ASSIGNER["iou_cost"]["weight"])
    for b, nv in enumerate(cfg["valid"]):
        rows = R.valid_rows(gt[b], cfg["C"])
        # the valid rows, compacted in ascending order
        assert out["num_valid"][b] == nv and np.array_equal(out["valid_map"][b, :nv], rows) and (out["valid_map"][b, nv:] == -1).all()
        # decode: the centres are the reference's bits, the rest lies inside its bound of the f64 evaluation
        box64, bound = R.decode_f64(preds, b)
        assert np.array_equal(out["boxes"][b, :, :3], g[f"{name}_boxes"][b, :, :3])
        d = np.abs(out["boxes"][b].astype(np.float64) - box64)
        print(f"{name}[{b}] decode ratio {(d / np.maximum(bound, 1e-300)).max():.3f}")
        assert (d <= bound).all()
        assert (out["cost"][b, :, nv:] == 0).all() and (out["iou"][b, :, nv:] == 0).all()
        if not nv:
            continue
        # iou: overlaps() composed in torch on the device-decoded boxes, the library's BEV overlap inside, bit for bit
        from findnpropagate_amd.iou3d_nms import iou3d_nms_cuda
        q, t = dev["boxes"][b], torch.from_numpy(gt[b, rows, :-1]).to(cuda)
        bev = torch.zeros((q.shape[0], t.shape[0]), device=cuda)
        iou3d_nms_cuda.boxes_overlap_bev_gpu(q[:, :7].contiguous(), t[:, :7].contiguous(), bev)
        top = torch.min((q[:, 2] + q[:, 5])[:, None], (t[:, 2] + t[:, 5])[None])
        bottom = torch.max(q[:, 2][:, None], t[:, 2][None])
        o3 = bev * torch.clamp(top - bottom, min=0)
        union = (q[:, 3] * q[:, 4] * q[:, 5])[:, None] + (t[:, 3] * t[:, 4] * t[:, 5])[None] - o3
        want_iou = (o3 / torch.clamp(union, min=1e-8)).cpu().numpy()
        assert np.array_equal(out["iou"][b, :, :nv].view(np.int32), want_iou.view(np.int32))
        assert (want_iou > 0.1).sum() >= min(nv, 3)
        # cost - iou_cost against cls + reg in f64, evaluated on the kernel's own decoded boxes
        gts = gt[b, rows]
        want, cb = R.cls_reg_f64(preds["heatmap"][b], out["boxes"][b].astype(np.float64), gts, gts[:, -1].astype(int) - 1)
        cost = out["cost"][b, :, :nv]
        lhs = cost.astype(np.float64) - (-(out["iou"][b, :, :nv]) * w_iou).astype(np.float64)
        cb = cb + R.U * np.abs(cost)
        print(f"{name}[{b}] cls + reg ratio {(np.abs(lhs - want) / cb).max():.3f}")
        assert (np.abs(lhs - want) <= cb).all()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_targets_end_to_end(cuda, name):
    g, preds, gt, out, _ = _fixture_run(cuda, name)
    cfg = R.CASES[name]
    want_assigned = np.full((len(cfg["valid"]), cfg["K"]), -1, np.int32)
    for b in range(len(cfg["valid"])):
        rows = R.valid_rows(gt[b], cfg["C"])
        if rows.size:
            want_assigned[b, g[f"{name}_match_rows{b}"]] = rows[g[f"{name}_match_cols{b}"]]
    assert np.array_equal(out["assigned"], want_assigned)
    for key in ("labels", "label_weights", "bbox_weights", "unknown_mask"):
        assert out[key].dtype == g[f"{name}_{key}"].dtype and np.array_equal(out[key], g[f"{name}_{key}"]), key
    assert int(out["num_pos"][0]) == int(g[f"{name}_num_pos"]) > 0
    for b in range(len(cfg["valid"])):
        pos = np.flatnonzero(want_assigned[b] >= 0)
        t64 = np.zeros((cfg["K"], cfg["code"]))
        tb = np.zeros_like(t64)
        if pos.size:
            t64[pos], tb[pos] = R.encode_f64(gt[b, want_assigned[b, pos], :-1])
        d = np.abs(out["bbox_targets"][b].astype(np.float64) - t64)
        print(f"{name}[{b}] encode ratio {(d / np.maximum(tb, 1e-300)).max():.3f}")
        assert (d <= tb).all()
        # matched IoU.  The value: exactly the kernel's own iou at the match, clamped (test_cost_kernel holds that iou to the torch
        # composition bit for bit).  Against the fixture: the kernel and the reference decode the query by different f32 routes and
        # iou_bound, a perimeter-times-displacement bound, is loose by construction; it guards the pairing, not the last digits.
        if pos.size:
            rows_ = R.valid_rows(gt[b], cfg["C"])
            own = np.clip(out["iou"][b, pos, np.searchsorted(rows_, want_assigned[b, pos])], 0.0, 1.0)
            assert np.array_equal(out["matched_ious"][b, pos].view(np.int32), own.view(np.int32))
            rows = R.valid_rows(gt[b], cfg["C"])
            box64, dbound = R.decode_f64(preds, b)
            cols = g[f"{name}_match_cols{b}"]
            q = g[f"{name}_match_rows{b}"]
            assert np.array_equal(q, pos)
            bev = torch.zeros((cfg["K"], rows.size))
            from findnpropagate_amd import lib
            a32, g32 = np.ascontiguousarray(box64[:, :7], np.float32), np.ascontiguousarray(gt[b, rows, :7])
            lib.check(lib.load().fnp_host_boxes_overlap_bev(a32.ctypes.data, cfg["K"], g32.ctypes.data, rows.size, bev.data_ptr()), "bev")
            ib = R.iou_bound(box64, gt[b, rows], bev.numpy().astype(np.float64), dbound)[q, cols]
            di = np.abs(out["matched_ious"][b, q].astype(np.float64) - g[f"{name}_matched_ious"][b, q])
            print(f"{name}[{b}] matched iou ratio {(di / np.maximum(ib, 1e-300)).max():.3f}, largest difference {di.max():.3e}")
            assert (di <= ib).all()
        neg = np.setdiff1d(np.arange(cfg["K"]), pos)
        assert (out["matched_ious"][b, neg] == 0).all()


def test_targets_of_padding_only(cuda):
    """a batch of only padding rows (and one of no rows at all): every query is background and num_pos is 0"""
    g, preds, gt, _, _ = _fixture_run(cuda, "main")
    heads = {h: torch.from_numpy(v).to(cuda) for h, v in preds.items()}
    for boxes in (torch.zeros((3, 48, 10), device=cuda), torch.zeros((3, 0, 10), device=cuda)):
        out = _query_targets("main")(heads, boxes)
        assert int(out["num_pos"][0]) == 0 and (out["labels"] == R.CASES["main"]["C"]).all() and (out["assigned"] == -1).all()
        assert (out["bbox_weights"] == 0).all() and (out["bbox_targets"] == 0).all() and (out["label_weights"] == 1).all()
        assert not out["unknown_mask"].any() and (out["matched_ious"] == 0).all()


def test_scene_alone_equals_scene_in_batch_and_runs_repeat(cuda):
    g, preds, gt, out, _ = _fixture_run(cuda, "main")
    qt = _query_targets("main")
    for b in (1, 2):
        alone = qt({h: torch.from_numpy(v[b:b + 1]).to(cuda) for h, v in preds.items()}, torch.from_numpy(gt[b:b + 1]).to(cuda),
                   return_debug=True)
        for key in ("cost", "iou", "boxes", "assigned", "labels", "bbox_targets", "bbox_weights", "matched_ious", "valid_map"):
            a, w = alone[key][0].cpu().numpy(), out[key][b]
            assert np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, w.view(np.int32) if w.dtype == np.float32 else w), key


def test_query_targets_read_nothing_back(cuda):
    g, preds, gt, out, _ = _fixture_run(cuda, "main")
    heads, boxes = {h: torch.from_numpy(v).to(cuda) for h, v in preds.items()}, torch.from_numpy(gt).to(cuda)
    qt = _query_targets("main")
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = qt(heads, boxes)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    for key in ("assigned", "labels", "bbox_targets", "matched_ious", "num_pos"):
        assert np.array_equal(again[key].cpu().numpy(), out[key]), key


# ---- the two query losses (fnp_tf_query_loss_forward / _backward) against the fixture's f64 run --------------------------------

def _loss_cfg(name, unknown=True):
    w = R.loss_weights(name)
    if not unknown:
        w = dict(code_weights=w["code_weights"])
    return dict(LOSS_CLS=dict(gamma=R.GAMMA, alpha=R.ALPHA), LOSS_WEIGHTS=w)


def _device_targets(cuda, targets):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(cuda) for k, v in targets.items() if k != "num_pos"}
    t["num_pos"] = torch.tensor([int(targets["num_pos"])], dtype=torch.int32, device=cuda)
    return t


def _run_loss(cuda, name, preds, targets, dtype=torch.float32, cfg=None):
    from findnpropagate_amd.utils.loss_utils import query_loss
    heads = ["heatmap"] + R.head_order(name)
    pp = {h: torch.from_numpy(preds[h]).to(cuda).to(dtype).requires_grad_(True) for h in heads}
    a, b = query_loss(pp, _device_targets(cuda, targets), cfg or _loss_cfg(name), R.head_order(name))
    assert a.dtype == torch.float32 and a.dim() == 0 and b.dim() == 0 and a.is_cuda
    (a + b).backward()
    return a.detach().cpu().numpy(), b.detach().cpu().numpy(), {h: pp[h].grad for h in heads}, pp


DTYPES = {"f32": (torch.float32, 0.0, 0.0), "f16": (torch.float16, 2.0 ** -11, 2.0 ** -25), "bf16": (torch.bfloat16, 2.0 ** -8, 0.0)}


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_query_loss_and_gradients(cuda, name, dtype):
    """Losses and every head gradient inside their bounds of the f64 evaluation (which IS the fixture's f64 run: CPU test).  f16 and
    bf16 heads are upcast exactly, so their reference is the f64 evaluation of the rounded inputs; their gradients are stored in
    the heads' dtype, which adds its half spacing (and, for f16, half its subnormal spacing) to the bound.  Two runs, same bits."""
    g = R.golden()
    dt, ulp, floor = DTYPES[dtype]
    heads = ["heatmap"] + R.head_order(name)
    preds = {h: g[f"{name}_pred_{h}"] for h in heads}
    targets = R.fixture_targets(name)
    a, b, grads, pp = _run_loss(cuda, name, preds, targets, dt)
    want = R.loss_f64(name, {h: pp[h].detach().double().cpu().numpy() for h in heads}, targets, out_ulp=ulp)
    if dtype == "f32":
        assert abs(want["loss_cls"] - g[f"{name}_f64_loss_cls"]) <= 1e-12 * want["loss_cls"]
    for key, v in (("loss_cls", a), ("loss_bbox", b)):
        ratio = abs(float(v) - want[key]) / want["bound_" + key]
        print(f"{name} {dtype} {key} ratio {ratio:.3f}")
        assert ratio <= 1
    for h in heads:
        assert grads[h].dtype == dt and grads[h].shape == pp[h].shape
        d = np.abs(grads[h].double().cpu().numpy() - want["grad_" + h])
        bound = want["bound_grad_" + h] + floor
        print(f"{name} {dtype} grad {h} ratio {(d / np.maximum(bound, 1e-300)).max():.3f}")
        assert (d <= bound).all()
    a2, b2, grads2, _ = _run_loss(cuda, name, preds, targets, dt)
    assert a2.tobytes() == a.tobytes() and b2.tobytes() == b.tobytes() and all(torch.equal(grads[h], grads2[h]) for h in heads)


def test_query_loss_without_positives_divides_by_one(cuda):
    g = R.golden()
    name, cfg = "main", R.CASES["main"]
    heads = ["heatmap"] + R.head_order(name)
    preds = {h: g[f"{name}_pred_{h}"] for h in heads}
    B, K = len(cfg["valid"]), cfg["K"]
    targets = dict(labels=np.full((B, K), cfg["C"], np.int64), label_weights=np.ones((B, K), np.float32),
                   bbox_targets=np.zeros((B, K, cfg["code"]), np.float32), bbox_weights=np.zeros((B, K, cfg["code"]), np.float32),
                   unknown_mask=np.zeros((B, K), bool), num_pos=np.int64(0))
    a, b, grads, _ = _run_loss(cuda, name, preds, targets)
    want = R.loss_f64(name, preds, targets)
    assert abs(float(a) - want["loss_cls"]) <= want["bound_loss_cls"] and want["loss_cls"] > 1 and float(b) == 0
    assert (np.abs(grads["heatmap"].double().cpu().numpy() - want["grad_heatmap"]) <= want["bound_grad_heatmap"]).all()
    assert all((grads[h] == 0).all() for h in R.head_order(name))


def test_query_loss_gradient_is_zero_where_prediction_equals_target(cuda):
    g = R.golden()
    name = "main"
    heads = ["heatmap"] + R.head_order(name)
    targets = dict(R.fixture_targets(name))
    targets["bbox_weights"] = np.ones_like(targets["bbox_weights"])
    targets["bbox_targets"] = np.random.default_rng(4).standard_normal(targets["bbox_targets"].shape).astype(np.float32)
    preds, at = {"heatmap": g[f"{name}_pred_heatmap"]}, 0
    for h in R.head_order(name):
        n = g[f"{name}_pred_{h}"].shape[1]
        preds[h] = np.ascontiguousarray(targets["bbox_targets"][:, :, at:at + n].transpose(0, 2, 1))
        at += n
    a, b, grads, _ = _run_loss(cuda, name, preds, targets)
    assert float(b) == 0 and all((grads[h] == 0).all() for h in R.head_order(name)) and (grads["heatmap"] != 0).any()
    preds["center"] = preds["center"].copy()
    preds["center"][1, 0, 7] += 1.0                                       # one element off its target: its gradient alone appears
    _, b, grads, _ = _run_loss(cuda, name, preds, targets)
    assert float(b) > 0 and int((grads["center"] != 0).sum()) == 1 and float(grads["center"][1, 0, 7]) > 0


def test_query_loss_unknown_weights_act_on_masked_queries_only(cuda):
    g = R.golden()
    name = "main"
    heads = ["heatmap"] + R.head_order(name)
    preds = {h: g[f"{name}_pred_{h}"] for h in heads}
    targets = R.fixture_targets(name)
    mask = torch.from_numpy(targets["unknown_mask"]).to(cuda)
    assert 2 <= int(mask.sum()) < mask.numel()
    _, _, with_w, _ = _run_loss(cuda, name, preds, targets)
    _, _, without, _ = _run_loss(cuda, name, preds, targets, cfg=_loss_cfg(name, unknown=False))
    for h in heads:
        same = (with_w[h] == without[h]).all(dim=1)                       # (B, K): every channel of the query
        assert same[~mask].all(), h
    assert not (with_w["heatmap"] == without["heatmap"]).all(dim=1)[mask].any()      # 0.4 scales every class gradient of a masked query
    assert not (with_w["dim"] == without["dim"]).all(dim=1)[mask].any()


def test_targets_and_losses_read_nothing_back(cuda):
    """QueryTargets + query_loss, forward and backward, with host synchronisation forbidden"""
    from findnpropagate_amd.utils.loss_utils import query_loss
    g, preds, gt, out, _ = _fixture_run(cuda, "main")
    heads = {h: torch.from_numpy(v).to(cuda).requires_grad_(True) for h, v in preds.items()}
    boxes, qt, cfg = torch.from_numpy(gt).to(cuda), _query_targets("main"), _loss_cfg("main")
    qt(heads, boxes)                                                      # (first use loads the code objects)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        t = qt(heads, boxes)
        a, b = query_loss(heads, t, cfg, R.head_order("main"))
        (a + b).backward()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    want = R.loss_f64("main", preds, R.fixture_targets("main"))
    assert abs(float(a) - want["loss_cls"]) <= want["bound_loss_cls"] and heads["rot"].grad is not None
