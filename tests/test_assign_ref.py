"""The restated solver equals scipy's linear_sum_assignment, rows and columns: the Python restatement (tests/ref_assign.py) and
the library's host entry point fnp_host_lsap (csrc/lsap.h), on random, tie-heavy and duplicated-column matrices of both
orientations; the fixture of the reference's get_targets is well separated and lies inside the derived bounds; the host BEV
overlap is the host IoU before its division.  No GPU."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import ref_assign as R
from findnpropagate_amd.dense_heads.transfusion_assign import lsap_host


def _check(solver, m):
    want_r, want_c = linear_sum_assignment(m)
    got_r, got_c = solver(m)
    assert np.array_equal(got_r, want_r) and np.array_equal(got_c, want_c), (m.shape, got_c.tolist(), want_c.tolist())


SOLVERS = {"restatement": R.lsap, "fnp_host_lsap": lsap_host}


@pytest.mark.parametrize("solver", sorted(SOLVERS))
@pytest.mark.parametrize("form", R.FORMS)
def test_random_rectangular_equals_scipy(solver, form):
    cases = R.random_rectangular(seed=R.FORMS.index(form), count=200, form=form)
    shapes = {(np.sign(m.shape[0] - m.shape[1])) for m in cases}
    assert shapes == {-1, 0, 1}                     # wide, square and tall (the transposed route) all occur
    for m in cases:
        _check(SOLVERS[solver], m)


@pytest.mark.parametrize("solver", sorted(SOLVERS))
@pytest.mark.parametrize("name", sorted(R.fixed_cases()))
def test_fixed_cases_equal_scipy(solver, name):
    m = R.fixed_cases()[name]
    _check(SOLVERS[solver], m)
    if "int" in name or "ties" in name:             # integers: the total cost is exact in any summation order
        r, c = SOLVERS[solver](m)
        wr, wc = linear_sum_assignment(m)
        assert m[r, c].astype(np.float64).sum() == m[wr, wc].astype(np.float64).sum()


def test_ties_make_the_assignment_ambiguous():
    """The tie-heavy cases do discriminate: another scan order (the columns reversed and mapped back) is as optimal as
    scipy's assignment, and is a different one."""
    m = R.fixed_cases()["200x60 int"]
    r, c = linear_sum_assignment(m)
    rr, cr = linear_sum_assignment(m[:, ::-1])
    cr = m.shape[1] - 1 - cr
    assert m[r, c].sum() == m[rr, cr].sum()
    assert not (np.array_equal(r, rr) and np.array_equal(c, cr))


def test_host_lsap_empty_and_non_finite():
    r, c = lsap_host(np.zeros((0, 5), np.float32))
    assert r.size == 0 and c.size == 0
    from findnpropagate_amd import lib
    bad = np.full((3, 4), np.inf, np.float32)
    with pytest.raises(lib.FnpError):
        lsap_host(bad)
    bad = np.full((4, 3), np.nan, np.float32)       # out of contract: must return, whatever it returns
    try:
        lsap_host(bad)
    except lib.FnpError:
        pass


# ---- the fixture (tests/golden/assign_golden.npz: the reference's get_targets on the CPU) and the bounds of ref_assign.py ---------

def _scene_arrays(name, b):
    g = R.golden()
    preds = {h: g[f"{name}_pred_{h}"] for h, _ in R.HEAD_DIMS if f"{name}_pred_{h}" in g}
    gt = g[f"{name}_gt_boxes"]
    rows = R.valid_rows(gt[b], R.CASES[name]["C"])
    return g, preds, gt, rows


SCENES = [(name, b) for name, cfg in R.CASES.items() for b in range(len(cfg["valid"]))]


def _host_bev(boxes, gts):
    from findnpropagate_amd import lib
    a, b = np.ascontiguousarray(boxes[:, :7], np.float32), np.ascontiguousarray(gts[:, :7], np.float32)
    out = np.zeros((a.shape[0], b.shape[0]), np.float32)
    lib.check(lib.load().fnp_host_boxes_overlap_bev(a.ctypes.data, a.shape[0], b.ctypes.data, b.shape[0], out.ctypes.data), "overlap")
    return out


@pytest.mark.parametrize("name,b", SCENES)
def test_reference_f32_run_lies_inside_the_bounds(name, b):
    """The bounds of ref_assign.py hold for the reference's own f32 CPU run (a bound it missed would be wrong): decoded boxes,
    cls + reg, and the encoded targets.  Prints the largest ratio of each."""
    g, preds, gt, rows = _scene_arrays(name, b)
    assert rows.size == R.CASES[name]["valid"][b]
    box64, bound = R.decode_f64(preds, b)
    got = g[f"{name}_boxes"][b].astype(np.float64)
    ratio = np.abs(got - box64) / np.maximum(bound, 1e-300)
    assert (np.abs(got - box64) <= bound).all(), ratio.max()
    print(f"{name}[{b}] decode ratio {ratio.max():.3f}")
    if rows.size:
        gts = gt[b, rows]
        want, cb = R.cls_reg_f64(preds["heatmap"][b], got, gts, gts[:, -1].astype(int) - 1)
        w = np.float32(R.ASSIGNER["iou_cost"]["weight"])
        lhs = g[f"{name}_cost{b}"].astype(np.float64) - (-(g[f"{name}_iou{b}"]) * w).astype(np.float64)
        cb = cb + R.U * np.abs(g[f"{name}_cost{b}"])
        assert (np.abs(lhs - want) <= cb).all(), (np.abs(lhs - want) / cb).max()
        print(f"{name}[{b}] cls + reg ratio {(np.abs(lhs - want) / cb).max():.3f}")
        pos = np.flatnonzero(g[f"{name}_labels"][b] < R.CASES[name]["C"])
        assert np.array_equal(pos, g[f"{name}_match_rows{b}"])
        src = rows[g[f"{name}_match_cols{b}"]]
        t64, tb = R.encode_f64(gt[b, src, :-1])
        code = R.CASES[name]["code"]
        d = np.abs(g[f"{name}_bbox_targets"][b, pos].astype(np.float64) - t64[:, :code])
        assert (d <= tb[:, :code]).all(), (d / np.maximum(tb[:, :code], 1e-300)).max()
        print(f"{name}[{b}] encode ratio {(d / np.maximum(tb[:, :code], 1e-300)).max():.3f}")


@pytest.mark.parametrize("name,b", [s for s in SCENES if R.CASES[s[0]]["valid"][s[1]]])
def test_fixture_scenes_are_well_separated(name, b):
    """The generator's condition, checked again from the stored arrays: scipy's match on the recorded f32 cost, on its f64
    evaluation and on 32 copies moved by +- the cost bound is one and the same; the restated solvers give it too."""
    g, preds, gt, rows = _scene_arrays(name, b)
    gts, cost, iou, cols = gt[b, rows], g[f"{name}_cost{b}"], g[f"{name}_iou{b}"], g[f"{name}_match_cols{b}"]
    box64, dbound = R.decode_f64(preds, b)
    clsreg, bound = R.cls_reg_f64(preds["heatmap"][b], box64, gts, gts[:, -1].astype(int) - 1)
    w = R.ASSIGNER["iou_cost"]["weight"]
    cost64 = clsreg - w * iou.astype(np.float64)
    bound = bound + w * R.iou_bound(box64, gts, _host_bev(box64, gts).astype(np.float64), dbound) + R.U * np.abs(cost64)
    assert np.array_equal(linear_sum_assignment(cost)[1], cols) and np.array_equal(linear_sum_assignment(cost64)[1], cols)
    rng = np.random.default_rng(5)
    for _ in range(32):
        moved = (cost.astype(np.float64) + rng.choice([-1.0, 1.0], cost.shape) * bound).astype(np.float32)
        assert np.array_equal(linear_sum_assignment(moved)[1], cols)
    assert np.array_equal(lsap_host(cost)[1], cols) and np.array_equal(R.lsap(cost)[1], cols)


def test_fixture_exact_outputs_follow_from_the_match():
    """labels, weights, masks and num_pos of the fixture are what the recorded match implies (the rule the target kernel
    implements), so the GPU test may compare them exactly."""
    g = R.golden()
    for name, cfg in R.CASES.items():
        gt, total = g[f"{name}_gt_boxes"], 0
        for b in range(len(cfg["valid"])):
            labels = np.full(cfg["K"], cfg["C"], np.int64)
            unknown = np.zeros(cfg["K"], bool)
            rows = R.valid_rows(gt[b], cfg["C"])
            if rows.size:
                q, src = g[f"{name}_match_rows{b}"], rows[g[f"{name}_match_cols{b}"]]
                labels[q] = gt[b, src, -1].astype(np.int64) - 1
                unknown[q] = np.isin(gt[b, src, -1].astype(int), cfg["unknown_labels"])
                total += q.size
            assert np.array_equal(g[f"{name}_labels"][b], labels) and np.array_equal(g[f"{name}_unknown_mask"][b], unknown)
            assert (g[f"{name}_label_weights"][b] == 1).all()
            assert np.array_equal(g[f"{name}_bbox_weights"][b], np.repeat((labels < cfg["C"])[:, None], cfg["code"], 1).astype(np.float32))
        assert int(g[f"{name}_num_pos"]) == total
        if cfg["unknown_labels"]:
            assert g[f"{name}_unknown_mask"].sum() >= 2


def test_host_overlap_is_the_host_iou_before_its_division(rng):
    """fnp_host_boxes_overlap_bev against fnp_host_boxes_iou_bev on the box generator of the host IoU tests: the IoU recomputed
    from the overlap by the IoU's own definition (f32, in its operand order) equals the library's IoU bit for bit."""
    from findnpropagate_amd import synthetic as syn
    from findnpropagate_amd.iou3d_nms import iou3d_nms_utils
    a, b = syn.random_boxes(rng, 64), syn.random_boxes(rng, 33)
    b[0], b[1, :2] = a[0], a[0, :2] + 100
    ov = _host_bev(a, b)
    iou = iou3d_nms_utils.boxes_bev_iou_cpu(a, b)
    sa, sb = (a[:, 3] * a[:, 4])[:, None], (b[:, 3] * b[:, 4])[None]
    assert np.array_equal(ov / np.maximum(sa + sb - ov, np.float32(1e-8)), np.asarray(iou))
    assert ov[0, 1] == 0 and ov[0, 0] == pytest.approx(float(sa[0, 0]), rel=1e-5) and (ov > 0).sum() > 10


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_plain_route_reproduces_the_fixture(name):
    """QueryTargets on CPU tensors takes the plain route (query_targets_plain): the discrete outputs and the match equal the
    reference's run exactly, the encoded boxes and the matched IoUs lie inside the derived bounds of its f64 evaluation."""
    import torch
    from findnpropagate_amd.dense_heads.transfusion_assign import QueryTargets
    g = R.golden()
    cfg = R.CASES[name]
    preds = {h: g[f"{name}_pred_{h}"] for h, _ in R.HEAD_DIMS if f"{name}_pred_{h}" in g}
    gt = g[f"{name}_gt_boxes"]
    qt = QueryTargets(dict(FEATURE_MAP_STRIDE=R.STRIDE, HUNGARIAN_ASSIGNER=R.ASSIGNER), R.RANGE, R.VOXEL, cfg["C"], code_size=cfg["code"],
                      unknown_labels=cfg["unknown_labels"])
    out = qt({h: torch.from_numpy(v) for h, v in preds.items()}, torch.from_numpy(gt), return_debug=True)
    for key in ("labels", "label_weights", "bbox_weights", "unknown_mask"):
        got = out[key].numpy()
        assert got.dtype == g[f"{name}_{key}"].dtype and np.array_equal(got, g[f"{name}_{key}"]), key
    assert int(out["num_pos"][0]) == int(g[f"{name}_num_pos"])
    for b, nv in enumerate(cfg["valid"]):
        rows = R.valid_rows(gt[b], cfg["C"])
        assert out["num_valid"][b] == nv and np.array_equal(out["valid_map"][b].numpy(), rows)
        want = np.full(cfg["K"], -1, np.int32)
        if nv:
            q, cols = g[f"{name}_match_rows{b}"], g[f"{name}_match_cols{b}"]
            want[q] = rows[cols]
            t64, tb = R.encode_f64(gt[b, rows[cols], :-1])
            assert (np.abs(out["bbox_targets"][b, q].numpy().astype(np.float64) - t64) <= tb).all()
            box64, dbound = R.decode_f64(preds, b)
            ib = R.iou_bound(box64, gt[b, rows], _host_bev(box64, gt[b, rows]).astype(np.float64), dbound)[q, cols]
            assert (np.abs(out["matched_ious"][b, q].numpy().astype(np.float64) - g[f"{name}_matched_ious"][b, q]) <= ib).all()
        assert np.array_equal(out["assigned"][b].numpy(), want)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_loss_bounds_hold_for_the_reference_and_the_plain_route(name):
    """The f64 evaluation of ref_assign.loss_f64 is the reference's own f64 run (losses and every head gradient, to 1e-12), the
    reference's f32 run lies inside the derived bounds, and query_loss_plain on CPU tensors does too, in f32, and equals the f64 run
    in f64."""
    import torch
    from findnpropagate_amd.utils.loss_utils import query_loss
    g = R.golden()
    preds = {h: g[f"{name}_pred_{h}"] for h, _ in R.HEAD_DIMS if f"{name}_pred_{h}" in g}
    targets = R.fixture_targets(name)
    want = R.loss_f64(name, preds, targets)
    own = R.loss_f64(name, preds, dict(targets, bbox_targets=g[f"{name}_f64_bbox_targets"]))     # on the f64 run's own targets
    heads = ["heatmap"] + R.head_order(name)
    for key in ("loss_cls", "loss_bbox"):
        assert abs(own[key] - g[f"{name}_f64_{key}"]) <= 1e-12 * abs(own[key])
        ratio = abs(g[f"{name}_f32_{key}"] - want[key]) / want["bound_" + key]
        print(f"{name} {key} reference f32 ratio {ratio:.3f}")
        assert ratio <= 1
    for h in heads:
        assert np.allclose(own["grad_" + h], g[f"{name}_f64_grad_{h}"], rtol=1e-12, atol=1e-300)
        d = np.abs(g[f"{name}_f32_grad_{h}"].astype(np.float64) - want["grad_" + h])
        print(f"{name} grad {h} reference f32 ratio {(d / np.maximum(want['bound_grad_' + h], 1e-300)).max():.3f}")
        assert (d <= want["bound_grad_" + h]).all()
    cfg = dict(LOSS_CLS=dict(gamma=R.GAMMA, alpha=R.ALPHA), LOSS_WEIGHTS=R.loss_weights(name))
    tt = {k: torch.from_numpy(np.asarray(v)) for k, v in targets.items()}
    tt["num_pos"] = torch.tensor([int(targets["num_pos"])], dtype=torch.int32)
    for dt, exact in ((torch.float32, False), (torch.float64, True)):
        pp = {h: torch.tensor(preds[h], dtype=dt, requires_grad=True) for h in heads}
        a, b = query_loss(pp, tt, cfg, R.head_order(name))
        (a + b).backward()
        for key, v in (("loss_cls", a), ("loss_bbox", b)):
            assert abs(float(v) - want[key]) <= (1e-12 * abs(want[key]) if exact else want["bound_" + key])
        for h in heads:
            d = np.abs(pp[h].grad.numpy().astype(np.float64) - want["grad_" + h])
            assert (d <= (1e-12 * np.abs(want["grad_" + h]) + 1e-300 if exact else want["bound_grad_" + h])).all(), h
