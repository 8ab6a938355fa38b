"""The adam_onecycle optimizer step on the CPU: tests/ref_optim.py (the f64 restatement of include/fnp.h's contract, its f32
roundoff bound and four wrong variants), the mirrored OneCycle / OptimWrapper and FusedAdamOneCycle's plain route, all held
to the reference's recorded run (tests/golden/adam_onecycle_golden.npz)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import optim_harness as H
import ref_optim as RO
from findnpropagate_amd.train_utils.optimization import (FusedAdamOneCycle, LossScaler, OneCycle, OptimWrapper, build_optimizer,
                                                         build_scheduler, layer_group_params)

G = RO.Golden()
CFG = {"OPTIMIZER": "adam_onecycle", "LR": 1e-3, "WEIGHT_DECAY": 0.01, "MOMS": [0.95, 0.85], "PCT_START": 0.4, "DIV_FACTOR": 10}
F64 = 1e-12     # f64 evaluations of the same formulas in another operand order: a few hundred ulps of slack, relative to the value's scale


def close64(got, want):
    for key in ("p", "m", "v"):
        for a, b in zip(got[key], want[key]):
            assert np.all(np.abs(a - b) <= F64 * np.maximum(np.abs(b), 1e-3 * np.abs(b).max(initial=0.0))), key
    assert np.array_equal(got["t"], want["t"])
    assert got["scale"] == want["scale"] and got["tracker"] == want["tracker"]


def golden_model():
    """the recorded run's model: its parameters in the optimizer's order are the record's tensors"""
    model = nn.Sequential(nn.Linear(6, 8), nn.BatchNorm1d(8), nn.Sequential(nn.Linear(8, 5), nn.BatchNorm1d(5)), nn.Linear(5, 4)).double()
    groups = layer_group_params(model)
    assert [len(g) for g in groups] == G.group_sizes and [p.numel() for p in groups[0] + groups[1]] == G.sizes
    with torch.no_grad():
        for p, a in zip(groups[0] + groups[1], RO.split(G.z["p0"], G.sizes)):
            p.copy_(torch.from_numpy(a).reshape(p.shape))
    return model


# ---------------------------------------------------------------------------------------------- the restatement and its bound
@pytest.mark.parametrize("k", range(G.K))
def test_ref_optim_matches_the_reference(k):
    new, norm, found = RO.step(G.state_before(k), G.grads(k), G.hp(k))
    close64(new, G.state_after(k))
    assert found == bool(G.z["found"][k])
    assert (norm == G.z["norm"][k]) if found else abs(norm - G.z["norm"][k]) <= F64 * norm


def test_the_record_is_what_the_issue_asks_for():
    z = G.z
    assert G.K == 13 and z["found"].tolist() == [0] * 5 + [1] + [0] * 7
    norms = z["norm"][:12]
    assert all(n < 3.5 for n in norms[0::2] if np.isfinite(n)) and all(n > 100 for n in norms[1::2] if np.isfinite(n))
    assert z["present"].sum() == z["present"].size - 1 and not z["present"][8, 2]
    assert len(set(z["scale_after"])) == 3 and (np.diff(z["scale_after"]) > 0).any() and (np.diff(z["scale_after"]) < 0).any()
    assert np.argmax(z["lr"][:12]) == 4 and z["mom"][0] == 0.95 and z["mom"][4] == 0.85       # both phases of the schedule
    assert np.load(RO.GOLDEN).files and all(v.dtype != object for v in z.values())


@pytest.mark.parametrize("variant", RO.VARIANTS)
def test_wrong_variant_lies_outside_the_bound(variant):
    ratios = []
    for k in range(G.K):
        before, grads, hp = G.state_before(k), G.grads(k), G.hp(k)
        wrong, _, _ = RO.step(before, grads, hp, variant=variant, beta1_first=float(G.z["mom"][0]))
        ratios.append(H.worst(wrong, G.state_after(k), RO.bound(before, grads, hp))[0])
    print(variant, ["%.3g" % r for r in ratios])
    assert max(ratios) > 1.0, (variant, ratios)


# ---------------------------------------------------------------------------------------------- the mirrors
def test_onecycle_sequences():
    class Fake:
        lr = mom = 0.0

    opt = Fake()
    sched = OneCycle(opt, 12, 1e-3, [0.95, 0.85], 10, 0.4)
    assert (opt.lr, opt.mom) == (1e-4, 0.95)
    for it in range(12):
        sched.step(it)
        for got, want in ((opt.lr, G.z["lr"][it]), (opt.mom, G.z["mom"][it])):
            assert abs(got - want) <= 2 * np.spacing(want), (it, got, want)       # numpy's cos may differ between builds


def reference_span(model, optimizer, scaler, max_norm):
    """tools/train_utils/train_utils.py:173-176"""
    scaler.unscale_(optimizer)
    torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
    scaler.step(optimizer)
    scaler.update()


def plain_state(optimizer, scaler, sizes):
    st = optimizer.state_dict()["state"]
    params = [p for g in optimizer.param_groups for p in g["params"]]
    z = lambda i: np.zeros(sizes[i])
    f = lambda key: [st[i][key].detach().double().numpy().reshape(-1) if i in st else z(i) for i in range(len(params))]
    return {"p": [p.detach().double().numpy().reshape(-1) for p in params], "m": f("exp_avg"), "v": f("exp_avg_sq"),
            "t": np.array([int(st[i]["step"]) if i in st else 0 for i in range(len(params))]),
            "scale": float(scaler.get_scale()), "tracker": int(scaler._growth_tracker.item())}


def test_mirrored_optimwrapper_follows_the_reference_in_f64():
    model = golden_model()
    optimizer = build_optimizer(model, CFG)
    assert isinstance(optimizer, OptimWrapper) and isinstance(optimizer.opt, torch.optim.Adam) and optimizer.true_wd
    sched, warm = build_scheduler(optimizer, 12, 1, -1, CFG)
    assert warm is None
    scaler = torch.amp.GradScaler("cpu", init_scale=float(G.z["scale_before"][0]), growth_interval=int(G.z["growth_interval"]))
    params = [p for g in optimizer.param_groups for p in g["params"]]
    for k in range(G.K):
        if k < 12:
            sched.step(k, 0)
        assert abs(optimizer.lr - G.z["lr"][k]) <= 2 * np.spacing(G.z["lr"][k])
        optimizer.zero_grad()
        scaler.scale(torch.zeros(()))
        for p, g in zip(params, G.grads(k)):
            p.grad = None if g is None else torch.from_numpy(g.copy()).reshape(p.shape)
        reference_span(model, optimizer, scaler, float(G.z["max_norm"][k]))
        close64(plain_state(optimizer, scaler, G.sizes), G.state_after(k))


# ---------------------------------------------------------------------------------------------- the fused class, plain route
def run_fused(dtype, round_inputs):
    """every record as ONE step from the record's state, and the 13 records as one trajectory -> per record (got, want, bound)"""
    prep_s = RO.as_f32 if round_inputs else (lambda s: s)
    prep_g = RO.grads_f32 if round_inputs else (lambda g: g)
    single = []
    for k in range(G.K):
        before, grads, hp = prep_s(G.state_before(k)), prep_g(G.grads(k)), G.hp(k)
        opt, scaler = H.fused_from_state(before, hp, G.group_sizes, dtype)
        assert "CPU tensors" in opt.fused_reasons()
        H.set_grads(opt, grads)
        opt.step_scaled(scaler, hp["max_norm"])
        want, norm, found = RO.step(before, grads, hp)
        assert int(opt.last_found_inf) == int(found)
        assert found or abs(float(opt.last_grad_norm) - norm) <= 2 * RO.U * norm
        single.append((H.read_state(opt, scaler), want, RO.bound(before, grads, hp)))
    trajectory = []
    ref = prep_s(G.state_before(0))
    opt, scaler = H.fused_from_state(ref, G.hp(0), G.group_sizes, dtype)
    carry = None
    for k in range(G.K):
        grads, hp = prep_g(G.grads(k)), G.hp(k)
        H.set_hp(opt, hp)
        H.set_grads(opt, grads)
        opt.step_scaled(scaler, hp["max_norm"])
        carry = RO.bound(ref, grads, hp, carry)
        ref, _, _ = RO.step(ref, grads, hp)
        trajectory.append((H.read_state(opt, scaler), ref, carry))
    assert opt.fused_steps == 0
    return single, trajectory


def test_fused_class_f64_on_cpu_follows_the_reference():
    single, trajectory = run_fused(torch.float64, round_inputs=False)
    for k in range(G.K):
        close64(single[k][0], G.state_after(k))
        close64(trajectory[k][0], G.state_after(k))


def test_fused_class_f32_on_cpu_stays_inside_the_bound():
    single, trajectory = run_fused(torch.float32, round_inputs=True)
    for name, runs in (("one step", single), ("trajectory", trajectory)):
        ratios = []
        for got, want, bounds in runs:
            ratios.append(H.worst(got, want, bounds)[0])
            assert np.array_equal(got["t"], want["t"]) and got["scale"] == want["scale"] and got["tracker"] == want["tracker"]
        print(name, "worst |err| / bound per record:", ["%.3f" % r for r in ratios])
        assert max(ratios) <= 1.0, (name, ratios)


def test_skipped_step_changes_nothing_and_halves_the_scale():
    k = 5
    before, hp = RO.as_f32(G.state_before(k)), G.hp(k)
    for with_scaler in (True, False):
        opt, scaler = H.fused_from_state(before if with_scaler else dict(before, scale=None), hp, G.group_sizes)
        grads = RO.grads_f32(G.grads(k))
        if not with_scaler:
            grads = [g / before["scale"] for g in grads]
        H.set_grads(opt, grads)
        was = H.raw_bits(opt)
        opt.step_scaled(scaler, hp["max_norm"])
        assert all(np.array_equal(a, b) for a, b in zip(was, H.raw_bits(opt)))
        assert int(opt.last_found_inf) == 1
        if with_scaler:
            assert scaler.get_scale() == before["scale"] * 0.5 and scaler.state_dict()["_growth_tracker"] == 0


def test_tensor_without_gradient_is_decayed_only():
    k, i = 8, 2
    before, hp = RO.as_f32(G.state_before(k)), G.hp(k)
    opt, scaler = H.fused_from_state(before, hp, G.group_sizes)
    H.set_grads(opt, RO.grads_f32(G.grads(k)))
    assert opt.params[i].grad is None
    opt.step_scaled(scaler, hp["max_norm"])
    got = H.read_state(opt, scaler)
    assert np.array_equal(got["m"][i], before["m"][i]) and np.array_equal(got["v"][i], before["v"][i])
    decay = np.float32(1.0 - hp["wd"] * hp["lr"])
    assert decay < 1 and np.array_equal(got["p"][i].astype(np.float32), before["p"][i].astype(np.float32) * decay)
    assert got["t"][i] == before["t"][i] and np.all(np.delete(got["t"], i) == np.delete(before["t"], i) + 1)
    assert got["t"][i] == got["t"].max() - 1


def test_scale_grows_at_the_interval():
    p = torch.ones(3, requires_grad=True)
    opt = FusedAdamOneCycle([[p], []], lr=1e-3, wd=0.0)
    scaler = LossScaler(True, init_scale=8.0, growth_interval=2)
    scales = []
    for _ in range(5):
        p.grad = torch.full((3,), 8.0)
        opt.step_scaled(scaler, 35.0)
        scales.append((scaler.get_scale(), scaler.state_dict()["_growth_tracker"]))
    assert scales == [(8.0, 1), (16.0, 0), (16.0, 1), (32.0, 0), (32.0, 1)]
    huge = LossScaler(True, init_scale=2.0 ** 127, growth_interval=1)       # growing would leave f32: the scale stays
    p.grad = torch.zeros(3)
    opt.step_scaled(huge, 35.0)
    assert huge.get_scale() == 2.0 ** 127 and huge.state_dict()["_growth_tracker"] == 0
    assert set(scaler.state_dict()) == set(torch.amp.GradScaler("cpu").state_dict())
    assert LossScaler(False).scale(p) is p and LossScaler(False).state_dict() == {}


def test_state_dict_round_trip_between_plain_and_fused():
    models = [golden_model(), golden_model()]
    plain = build_optimizer(models[0], CFG)
    fused = build_optimizer(models[1], dict(CFG, FNP_FUSED_STEP=True))
    assert isinstance(fused, FusedAdamOneCycle) and fused.group_sizes == G.group_sizes
    scheds = [build_scheduler(o, 12, 1, -1, CFG)[0] for o in (plain, fused)]
    plist = [p for g in plain.param_groups for p in g["params"]]

    def both_step(k):
        for s in scheds:
            s.step(k, 0)
        for params in (plist, fused.params):
            for p, g in zip(params, G.grads(k)):
                p.grad = None if g is None else torch.from_numpy(g / G.z["scale_before"][k]).reshape(p.shape)
        torch.nn.utils.clip_grad_norm_(plist, 35.0)
        plain.step()
        fused.step_scaled(None, 35.0)

    def same():
        a, b = plain.state_dict(), fused.state_dict()
        assert a["state"].keys() == b["state"].keys()
        assert [g.keys() for g in a["param_groups"]] == [g.keys() for g in b["param_groups"]]
        assert [g["params"] for g in a["param_groups"]] == [g["params"] for g in b["param_groups"]]
        for i in a["state"]:
            assert float(a["state"][i]["step"]) == float(b["state"][i]["step"])
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.allclose(a["state"][i][key], b["state"][i][key], rtol=F64, atol=0)
        for p, q in zip(plist, fused.params):
            assert torch.allclose(p, q, rtol=1e-11, atol=0)

    for k in (0, 1, 8):         # (record 8: tensor 2 has no gradient, so its step count falls behind)
        both_step(k)
    same()
    # plain -> fused
    fresh = FusedAdamOneCycle([fused.params[:G.group_sizes[0]], fused.params[G.group_sizes[0]:]], wd=0.01)
    fresh.load_state_dict(copy.deepcopy(plain.state_dict()))
    assert fresh.steps.tolist() == fused.steps.tolist() and (fresh.lr, fresh.mom, fresh.beta) == (plain.lr, plain.mom, plain.beta)
    assert all(torch.equal(a, b) for a, b in zip(fresh.exp_avg + fresh.exp_avg_sq, [plain.state_dict()["state"][i][key]
               for key in ("exp_avg", "exp_avg_sq") for i in range(len(plist))]))
    # fused -> plain: a fresh mirror takes the fused state and goes on as the fused class does
    plain2 = build_optimizer(models[0], CFG)
    plain2.load_state_dict(copy.deepcopy(fused.state_dict()))
    plain2.wd = 0.01
    plain = plain2
    scheds[0] = build_scheduler(plain, 12, 1, -1, CFG)[0]
    for k in (9, 10):
        both_step(k)
    same()


# ---------------------------------------------------------------------------------------------- what reaches the library
def test_steady_step_is_one_library_call(monkeypatch):
    import launch_trace as LT

    lengths = [5, 0, 9000]
    params = [torch.zeros(n, requires_grad=True) for n in lengths]
    opt = FusedAdamOneCycle([params[:2], params[2:]], wd=0.01, chunk=4096)
    monkeypatch.setattr(FusedAdamOneCycle, "fused_reasons", lambda self: [])
    scaler = LossScaler(True, 4.0)
    for p in params[:2]:
        p.grad = torch.zeros_like(p)
    with LT.installed() as rec:
        opt.step_scaled(scaler, 35.0)
        first = rec.take()
        opt.zero_grad()
        opt.step_scaled(scaler, 35.0)
        second = rec.take()
        params[2].grad = torch.zeros_like(params[2])
        opt.step()
        third = rec.take()
    assert [c[0] for c in first] == [c[0] for c in second] == [c[0] for c in third] == ["fnp_adam_onecycle_step"]
    assert opt.uploads == 2 and opt.fused_steps == 3       # the table went up at the first step and when a gradient appeared
    assert first[0][1:3] == [3, 4] and first[0][3] == [[4, 16], "uint8", False]      # chunks: 1 + 0 + 3
    table = opt._table.tolist()
    assert table[:3] == [p.data_ptr() for p in params] and table[3:6] == [p.grad.data_ptr() or opt.steps.data_ptr() for p in params]
    assert second[0][9:11] == [[[1], "float32", False], [[1], "int32", False]] and third[0][9:11] == [None, None]
    assert third[0][16] == float("inf")


def test_a_gradient_rebound_at_the_same_address_is_checked_again(monkeypatch):
    import launch_trace as LT

    real = FusedAdamOneCycle.fused_reasons
    monkeypatch.setattr(FusedAdamOneCycle, "fused_reasons", lambda self: [r for r in real(self) if r != "CPU tensors"])
    p = torch.ones(4, 4, requires_grad=True)
    opt = FusedAdamOneCycle([[p], []], wd=0.01)
    storage = torch.ones(4, 4)
    with LT.installed() as rec:
        p.grad = storage
        opt.step()
        assert [c[0] for c in rec.take()] == ["fnp_adam_onecycle_step"] and opt.fused_steps == 1
        p.grad = storage.t()            # the same address and shape, another stride: not what the kernels stream
        assert p.grad.data_ptr() == storage.data_ptr() and not p.grad.is_contiguous()
        opt.step()
        assert rec.take() == [] and opt.fused_steps == 1 and opt.steps.tolist() == [1]      # (the recorder's first step wrote nothing)
        p.grad = storage
        opt.step()
        assert [c[0] for c in rec.take()] == ["fnp_adam_onecycle_step"] and opt.fused_steps == 2


def test_a_half_precision_loss_is_scaled_in_f32():
    scaler = LossScaler(True)                                   # 2^16, the reference's default: no half holds it
    loss = torch.tensor(1.5, dtype=torch.float16)
    out = scaler.scale(loss)
    want = torch.amp.GradScaler("cpu").scale(torch.tensor(1.5, dtype=torch.float16))
    assert out.dtype == want.dtype == torch.float32 and out.shape == want.shape == () and float(out) == float(want) == 1.5 * 2.0 ** 16
    scaler.load_state_dict(dict(scaler.state_dict(), scale=4.0))
    assert float(scaler.scale(torch.tensor([2.0, 3.0])).sum()) == 20.0


def test_non_finite_hyper_parameters_are_refused_before_any_launch():
    import ctypes

    from findnpropagate_amd import lib

    L = lib.load()
    word = (ctypes.c_int64 * 4)()
    at = ctypes.addressof(word)

    def call(lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8, wd=0.01, max_norm=35.0, growth=2.0, backoff=0.5, interval=2000, scale=at):
        return L.fnp_adam_onecycle_step(0, 0, None, None, None, None, None, None, scale, at if scale else None, lr, beta1, beta2, eps, wd,
                                        max_norm, growth, backoff, interval, at, 32, at, at, None)

    inf, nan = float("inf"), float("nan")
    for bad in ({"lr": inf}, {"lr": -inf}, {"lr": nan}, {"wd": inf}, {"wd": nan}, {"eps": inf}, {"eps": -1e-8}, {"eps": nan}, {"beta1": 1.0},
                {"beta2": -0.1}, {"beta1": nan}, {"max_norm": -1.0}, {"max_norm": nan}, {"growth": inf}, {"backoff": 0.0}, {"interval": 0}):
        assert call(**bad) == -1, bad       # FNP_ERR_ARG
    assert call(lr=inf, scale=None) == -1
    assert list(word) == [0, 0, 0, 0]
