"""Between tests/ref_optim.py's states (numpy) and the library's FusedAdamOneCycle / LossScaler (torch): shared by
tests/test_optim_ref.py (CPU) and tests/test_gpu_optim.py."""
import numpy as np
import torch

import ref_optim as RO
from findnpropagate_amd.train_utils.optimization import FusedAdamOneCycle, LossScaler


def make_params(arrays, dtype, device, view_of=()):
    """leaf tensors of the arrays' values; those listed in view_of are views that start 4 bytes behind a 16-byte boundary"""
    out = []
    for i, a in enumerate(arrays):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
        if i in view_of:
            base = torch.zeros(a.size + 8, dtype=dtype, device=device)
            skip = ((16 - base.data_ptr() % 16) % 16) // base.element_size() + 1
            p = base[skip:skip + a.size]
            p.copy_(t)
            assert p.data_ptr() % 16 == base.element_size()
        else:
            p = t.to(device)
        out.append(p.requires_grad_(True))
    return out


def fused_from_state(state, hp, group_sizes, dtype=torch.float32, device="cpu", view_of=(), chunk=None):
    """(optimizer, scaler or None) holding `state` with the hyper-parameters of `hp`"""
    params = make_params(state["p"], dtype, device, view_of)
    g0 = group_sizes[0]
    kw = {} if chunk is None else {"chunk": chunk}
    opt = FusedAdamOneCycle([params[:g0], params[g0:]], lr=hp["lr"], wd=hp["wd"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], **kw)
    with torch.no_grad():
        for dst, src in zip(opt.exp_avg + opt.exp_avg_sq, list(state["m"]) + list(state["v"])):
            dst.copy_(torch.from_numpy(np.ascontiguousarray(src)).to(dtype))
        opt.steps.copy_(torch.from_numpy(np.asarray(state["t"], np.int32)))
    scaler = None
    if state["scale"] is not None:
        scaler = LossScaler(True, state["scale"], hp["growth_factor"], hp["backoff_factor"], hp["growth_interval"])
        scaler.load_state_dict(dict(scaler.state_dict(), _growth_tracker=state["tracker"]))
    return opt, scaler


def set_hp(opt, hp):
    opt.lr, opt.mom, opt.beta, opt.wd = hp["lr"], hp["beta1"], hp["beta2"], hp["wd"]


def set_grads(opt, grads):
    """assign the gradients, in place where a parameter has one already (its address stays)"""
    for p, g in zip(opt.params, grads):
        if g is None:
            p.grad = None
            continue
        with np.errstate(over="ignore"):
            t = torch.from_numpy(np.ascontiguousarray(g)).to(p.dtype).reshape(p.shape)
        if p.grad is None:
            p.grad = t.to(p.device)
        else:
            p.grad.copy_(t)


def read_state(opt, scaler):
    f = lambda ts: [t.detach().cpu().double().numpy().reshape(-1).copy() for t in ts]
    return {"p": f(opt.params), "m": f(opt.exp_avg), "v": f(opt.exp_avg_sq), "t": opt.steps.cpu().numpy().astype(np.int64),
            "scale": None if scaler is None else scaler.get_scale(),
            "tracker": 0 if scaler is None else scaler.state_dict()["_growth_tracker"]}


def raw_bits(opt):
    """p, m, v as they lie (their own dtype) and t: for array_equal"""
    return [t.detach().cpu().numpy().copy() for t in opt.params + opt.exp_avg + opt.exp_avg_sq] + [opt.steps.cpu().numpy().copy()]


def worst(got, want, bounds):
    """the largest |got - want| / bound over p, m, v (0/0 counts as 0), and where"""
    top = (0.0, None)
    for key, d in zip(("p", "m", "v"), bounds):
        for i, (a, b, lim) in enumerate(zip(got[key], want[key], d)):
            if a.size == 0:
                continue
            with np.errstate(invalid="ignore", divide="ignore"):
                err = np.abs(a - b)
                ratio = np.where(err == 0, 0.0, err / lim)
            ratio = np.where(np.isfinite(a) & np.isfinite(b), ratio, np.inf)
            if ratio.max() > top[0]:
                top = (float(ratio.max()), (key, i, int(ratio.argmax())))
    return top
