#!/usr/bin/env python3
"""Golden trajectory for the adam_onecycle optimizer step by RUNNING THE REFERENCE on the CPU, on f64 parameters:
tools/train_utils/optimization (build_optimizer, build_scheduler, OptimWrapper.step over torch's Adam) inside the span of
tools/train_utils/train_utils.py:156-176 (lr_scheduler.step, zero_grad, GradScaler.scale / unscale_, clip_grad_norm_,
scaler.step, scaler.update).  The gradients are not a model's: they are assigned, scaled by the scaler's scale as
scaler.scale(loss).backward() would leave them.

Runs in the build container only (needs the reference).  The reference modules are imported from where they lie.
Output: tests/golden/adam_onecycle_golden.npz (arrays only); tests/ref_optim.py reads it back.

The record: 12 iterations over a OneCycle of 12 total steps at the shipped hyper-parameters (transfusion_lidar.yaml: LR 1e-3,
MOMS [0.95, 0.85], PCT_START 0.4, DIV_FACTOR 10, BETAS default, WEIGHT_DECAY 0.01, GRAD_NORM_CLIP 35), the gradient norms
alternating between about 1 and about 300, an inf in one gradient at iteration 5, one tensor without a gradient at
iteration 8, growth_interval 3.  A 13th record follows them: one more step from the state after iteration 11 at iteration
11's lr and beta1, with max_norm 1e-3 on a gradient of norm about 2e-3.  At max_norm 35 the 1e-6 of the clip's denominator
changes the clipped gradient by less than 3e-8 of itself, under f32's unit roundoff: no f32 bound can tell a clip without it
from a clip with it there, and this record is what can."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("FNP_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "tools", "train_utils"))

import optimization as ref_opt  # noqa: E402  (the reference's package)
from torch.nn.utils import clip_grad_norm_  # noqa: E402  (what train_utils.py imports)


class Cfg(dict):
    __getattr__ = dict.__getitem__


CFG = Cfg(OPTIMIZER="adam_onecycle", LR=1e-3, WEIGHT_DECAY=0.01, MOMENTUM=0.9, MOMS=[0.95, 0.85], PCT_START=0.4, DIV_FACTOR=10,
          DECAY_STEP_LIST=[35, 45], LR_DECAY=0.1, LR_CLIP=1e-7, LR_WARMUP=False, WARMUP_EPOCH=1, GRAD_NORM_CLIP=35)
STEPS, INF_AT, NONE_AT, NONE_TENSOR, GROWTH_INTERVAL, INIT_SCALE = 12, 5, 8, 2, 3, 2.0 ** 10
SIDE_MAX_NORM = 1e-3


def make_model(rng):
    model = nn.Sequential(nn.Linear(6, 8), nn.BatchNorm1d(8), nn.Sequential(nn.Linear(8, 5), nn.BatchNorm1d(5)), nn.Linear(5, 4)).double()
    with torch.no_grad():
        for i, p in enumerate(model.parameters()):      # magnitudes 1 and 1e-3 in turn: where |p| is small the update is not
            p.copy_(torch.from_numpy(rng.normal(size=tuple(p.shape)) * (1.0 if i % 2 == 0 else 1e-3)))
    return model


def main():
    rng = np.random.default_rng(20261021)
    model = make_model(rng)
    optimizer = ref_opt.build_optimizer(model, CFG)
    lr_scheduler, _ = ref_opt.build_scheduler(optimizer, total_iters_each_epoch=STEPS, total_epochs=1, last_epoch=-1, optim_cfg=CFG)
    scaler = torch.amp.GradScaler("cpu", enabled=True, init_scale=INIT_SCALE, growth_interval=GROWTH_INTERVAL)
    params = [p for g in optimizer.param_groups for p in g["params"]]       # the optimizer's order: non-BatchNorm, BatchNorm
    sizes = [p.numel() for p in params]
    flat = lambda ts: np.concatenate([t.detach().numpy().reshape(-1) for t in ts])
    rec = {k: [] for k in ("lr", "mom", "max_norm", "scale_before", "tracker_before", "grads", "present", "p", "m", "v", "t",
                           "scale_after", "tracker_after", "norm", "found")}
    out = {"sizes": np.array(sizes, np.int64), "group_sizes": np.array([len(g["params"]) for g in optimizer.param_groups], np.int64),
           "p0": flat(params), "beta2": np.float64(optimizer.beta), "eps": np.float64(optimizer.param_groups[0]["eps"]),
           "wd": np.float64(CFG.WEIGHT_DECAY), "growth_interval": np.int64(GROWTH_INTERVAL), "growth_factor": np.float64(2.0),
           "backoff_factor": np.float64(0.5)}
    for it in range(STEPS + 1):
        side = it == STEPS
        if not side:
            lr_scheduler.step(it, 0)
        max_norm = SIDE_MAX_NORM if side else CFG.GRAD_NORM_CLIP
        optimizer.zero_grad()
        scaler.scale(torch.zeros(()))        # (makes the scaler's tensors, as scaler.scale(loss) does)
        scale = float(scaler.get_scale())
        rec["scale_before"].append(scale)
        rec["tracker_before"].append(int(scaler._growth_tracker.item()))
        target = 2e-3 if side else (1.0 if it % 2 == 0 else 300.0)
        raw = [rng.normal(size=tuple(p.shape)) for p in params]
        gain = target / np.sqrt(sum((g ** 2).sum() for g in raw))
        present = np.ones(len(params), bool)
        for i, (p, g) in enumerate(zip(params, raw)):
            g = g * gain * scale
            if it == INF_AT and i == 4:
                g.reshape(-1)[1] = np.inf
            if it == NONE_AT and i == NONE_TENSOR:
                present[i], p.grad, raw[i] = False, None, np.zeros_like(g)
                continue
            p.grad, raw[i] = torch.from_numpy(g.copy()), g
        rec["grads"].append(np.concatenate([g.reshape(-1) for g in raw]))
        rec["present"].append(present)
        # train_utils.py:173-176
        scaler.unscale_(optimizer)
        norm = clip_grad_norm_(model.parameters(), max_norm)
        found = sum(v.item() for v in scaler._per_optimizer_states[id(optimizer)]["found_inf_per_device"].values())
        scaler.step(optimizer)
        scaler.update()
        state = optimizer.state_dict()["state"]
        zeros = lambda i: torch.zeros(sizes[i], dtype=torch.float64)
        rec["lr"].append(float(optimizer.lr)); rec["mom"].append(float(optimizer.mom)); rec["max_norm"].append(float(max_norm))
        rec["p"].append(flat(params))
        rec["m"].append(flat([state[i]["exp_avg"] if i in state else zeros(i) for i in range(len(params))]))
        rec["v"].append(flat([state[i]["exp_avg_sq"] if i in state else zeros(i) for i in range(len(params))]))
        rec["t"].append(np.array([int(state[i]["step"]) if i in state else 0 for i in range(len(params))], np.int64))
        rec["scale_after"].append(float(scaler.get_scale())); rec["tracker_after"].append(int(scaler._growth_tracker.item()))
        rec["norm"].append(float(norm)); rec["found"].append(int(found > 0))
    out.update({k: np.array(v) for k, v in rec.items()})
    path = os.path.join(HERE, "adam_onecycle_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; found", out["found"].tolist(), "scale", out["scale_after"].tolist(),
          "norm", np.round(out["norm"], 4).tolist(), "t", out["t"][-1].tolist())


if __name__ == "__main__":
    main()
