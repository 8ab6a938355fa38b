"""The device heatmap proposals (fnp_proposals) and query initialisation (fnp_query_init) of TransFusionHead against the
reference's own output (tests/golden/proposals_golden.npz) where the reference's order is defined, and against
tests/ref_proposals.py (held to that fixture by tests/test_proposals_ref.py) in the tie, zero-fill and refinement cases.
Everything is exact except the fused sigmoid's scores, which are held to the f64 sigmoid inside the bound of ref_proposals."""
import os

import numpy as np
import pytest
import torch

import ref_proposals as RP

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proposals_golden.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def restated():
    return {name: RP.proposals(RP.case_map(name), c) for name, c in RP.CASES.items() if not c["exact"]}


def make(name):
    from findnpropagate_amd.dense_heads.transfusion_proposals import HeatmapProposals

    c = RP.CASES[name]
    return HeatmapProposals(c["K"], 3, c["C"], c["dataset_name"], c["class_names"])


def run(name, dev, x=None, from_logits=None):
    """-> top_class, top_index, top_score, qhs as numpy; the outputs are prefilled with -1 / NaN: an unwritten element shows"""
    c = RP.CASES[name]
    x = RP.case_map(name) if x is None else x
    B, K = x.shape[0], c["K"]
    out = (torch.full((B, K), -1, dtype=torch.int64, device=dev), torch.full((B, K), -1, dtype=torch.int64, device=dev),
           torch.full((B, K), float("nan"), device=dev), torch.full((B, c["C"], K), float("nan"), device=dev))
    got = make(name)(torch.from_numpy(x).to(dev), from_logits=c["from_logits"] if from_logits is None else from_logits, out=out)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    got = [g.cpu().numpy() for g in got]
    assert (got[0] >= 0).all() and (got[1] >= 0).all() and not np.isnan(got[2]).any() and not np.isnan(got[3]).any()
    return got


@pytest.mark.parametrize("name", [n for n, c in RP.CASES.items() if c["exact"] and not c["from_logits"]])
def test_equal_to_reference(cuda, gold, name):
    """small map (B = 1, 3), borders, Waymo and kitti masks, full size (K = 200, 500)"""
    top_class, top_index, top_score, qhs = run(name, cuda)
    assert np.array_equal(top_class, gold[name + "_top_class"])
    assert np.array_equal(top_index, gold[name + "_top_index"])
    assert np.array_equal(qhs, gold[name + "_qhs"])
    assert np.array_equal(top_score, np.take_along_axis(qhs, top_class[:, None, :], axis=1)[:, 0])


def test_border_peaks(cuda):
    top_class, top_index, top_score, _ = run("borders", cuda)
    W = RP.CASES["borders"]["W"]
    c, h, w = RP.BORDER_POINT
    assert (top_class[0, 0], top_index[0, 0], top_score[0, 0]) == (c, h * W + w, np.float32(0.98))
    c, h, w = RP.BORDER_ORDINARY
    assert not ((top_class[0] == c) & (top_index[0] == h * W + w)).any()


@pytest.mark.parametrize("name", [n for n, c in RP.CASES.items() if not c["exact"]])
def test_ties_zero_fill_and_refinement_equal_restatement(cuda, restated, name):
    got = run(name, cuda)
    for g, w, what in zip(got, restated[name], ("top_class", "top_index", "top_score", "query_heatmap_score")):
        if name == "zerofill" and what in ("top_score", "query_heatmap_score"):
            continue                                                 # (a fused sigmoid: held below)
        assert np.array_equal(g, w), what
    if name == "zerofill":                                          # sigmoid(-200) is exactly 0; the 37 cells within the bound
        x = RP.case_map(name)
        c = RP.CASES[name]
        flat = got[0] * (c["H"] * c["W"]) + got[1]
        logit = np.take_along_axis(x.reshape(c["B"], -1), flat, axis=1).astype(np.float64)
        positive = restated[name][2] > 0
        assert np.array_equal(got[2] > 0, positive) and (got[2][~positive] == 0).all()
        assert RP.ulps(got[2][positive], 1 / (1 + np.exp(-logit[positive]))).max() <= RP.SIGMOID_FIRST_ORDER_ULP
        assert np.array_equal(got[3] > 0, restated[name][3] > 0)


def test_fused_sigmoid(cuda, gold):
    """selection exact against the fixture (neighbouring sigmoids are >= 780 ulps apart); scores within
    sigmoid_ref_ulp (the reference's own f32 error, from the fixture) + 2 ulps of the f64 sigmoid of the f32 logit"""
    name = "sigmoid"
    c = RP.CASES[name]
    x = RP.case_map(name)
    top_class, top_index, top_score, qhs = run(name, cuda)
    assert np.array_equal(top_class, gold[name + "_top_class"]) and np.array_equal(top_index, gold[name + "_top_index"])
    bound = float(gold["sigmoid_ref_ulp"][0]) + RP.SIGMOID_EXTRA_ULP
    flat = top_class * (c["H"] * c["W"]) + top_index
    want = 1 / (1 + np.exp(-np.take_along_axis(x.reshape(1, -1), flat, axis=1).astype(np.float64)))
    err = RP.ulps(top_score, want).max()
    print(f"fused sigmoid: {err:.3f} ulp against f64 (bound {bound:.3f})")
    assert err <= bound
    ref = gold[name + "_qhs"]
    assert np.array_equal(qhs > 0, ref > 0)
    nz = ref > 0
    all_classes = 1 / (1 + np.exp(-x.reshape(1, c["C"], -1)[0][:, top_index[0]].astype(np.float64)))[None]
    assert RP.ulps(qhs[nz], all_classes[nz]).max() <= bound
    assert np.array_equal(top_score, np.take_along_axis(qhs, top_class[:, None, :], axis=1)[:, 0])
    # the probability path on the device's own sigmoid output: same selection
    again = run(name, cuda, x=torch.from_numpy(x).sigmoid().numpy(), from_logits=False)
    assert np.array_equal(again[0], top_class) and np.array_equal(again[1], top_index)


def test_run_to_run(cuda):
    for name in ("ties", "refine", "small_b3"):
        a, b = run(name, cuda), run(name, cuda)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_infinite_logits(cuda):
    name = "sigmoid"
    x = RP.case_map(name).copy()
    x[0, 2, 10, 10], x[0, 8, 0, 0], x[0, 4, 5, 5] = np.inf, np.inf, -np.inf
    top_class, top_index, top_score, _ = run(name, cuda, x=x)
    W = RP.CASES[name]["W"]
    assert top_score[0, :2].tolist() == [1.0, 1.0]
    assert list(zip(top_class[0, :2].tolist(), top_index[0, :2].tolist())) == [(2, 10 * W + 10), (8, 0)]
    assert not ((top_class[0] == 4) & (top_index[0] == 5 * W + 5)).any()


def test_empty_batch(cuda):
    c = RP.CASES["small_b1"]
    got = make("small_b1")(torch.zeros((0, c["C"], c["H"], c["W"]), device=cuda))
    assert [tuple(g.shape) for g in got] == [(0, c["K"]), (0, c["K"]), (0, c["K"]), (0, c["C"], c["K"])]
    assert got[0].dtype == torch.int64 and got[2].dtype == torch.float32


def query_case(gold, dev):
    name = RP.QUERY_CASE
    c = RP.CASES[name]
    feat, w, bias = RP.query_inputs(name)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return (t(feat.reshape(c["B"], RP.QUERY_FEATURES, -1)), t(gold[name + "_bev_pos"]), t(w), t(bias), t(gold[name + "_top_class"]),
            t(gold[name + "_top_index"]))


def test_init_queries_equal_reference(cuda, gold):
    name = RP.QUERY_CASE
    head = make(name)
    feat, pos, w, bias, cls, idx = query_case(gold, cuda)
    with torch.no_grad():
        for table in (pos, pos[None], pos[None].repeat(feat.shape[0], 1, 1)):
            qf, qp = head.init_queries(feat, table, w, bias, cls, idx)
            assert torch.equal(qf.cpu(), torch.from_numpy(gold[name + "_query_feat"]))
            assert torch.equal(qp.cpu(), torch.from_numpy(gold[name + "_query_pos"]))
    # on the device's own proposals as well (the same indices: the case is exact)
    top_class, top_index, _, _ = head(torch.from_numpy(RP.case_map(name)).to(cuda), from_logits=False)
    qf, _ = head.init_queries(feat, pos, w, bias, top_class, top_index)
    assert torch.equal(qf.cpu(), torch.from_numpy(gold[name + "_query_feat"]))
    bad = idx.clone()
    bad[0, 0] = feat.shape[2]                                       # out of range: NaN, never followed
    qf, qp = head.init_queries(feat, pos, w, bias, cls, bad)
    assert torch.isnan(qf[0, :, 0]).all() and torch.isnan(qp[0, 0]).all() and not torch.isnan(qf[0, :, 1:]).any()


def test_init_queries_grad_path(cuda, gold):
    """with autograd recording, the wrapper runs the plain span on the given indices: values and gradients are the mirror's"""
    from findnpropagate_amd.dense_heads.transfusion_proposals import init_queries_plain

    head = make(RP.QUERY_CASE)
    feat, pos, w, bias, cls, idx = query_case(gold, cuda)
    # small integers as the upstream gradient: a cell chosen by several queries sums their gradients with float atomics in any
    # order (torch's gather backward), and sums of small integers are exact in every order, so equality is well defined
    g = torch.from_numpy(np.random.default_rng(0).integers(-8, 9, (feat.shape[0], RP.QUERY_FEATURES, idx.shape[1])).astype(np.float32)).to(cuda)
    grads = []
    for fn in (head.init_queries, init_queries_plain):
        leaves = [t.clone().requires_grad_(True) for t in (feat, w, bias)]
        qf, qp = fn(leaves[0], pos, leaves[1], leaves[2], cls, idx)
        assert qf.requires_grad
        (qf * g).sum().backward()
        grads.append([qf.detach()] + [t.grad for t in leaves])
    for a, b in zip(*grads):
        assert torch.equal(a, b)
    assert torch.equal(grads[0][0].cpu(), torch.from_numpy(gold[RP.QUERY_CASE + "_query_feat"]))
