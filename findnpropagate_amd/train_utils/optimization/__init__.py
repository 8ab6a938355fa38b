"""The reference's tools/train_utils/optimization for its `adam_onecycle` recipe: build_optimizer and build_scheduler with the
reference's signatures.  `optim_cfg` is the reference's OPTIMIZATION node (attribute access and .get, an EasyDict there) or a
plain dict with the same keys.

    optimizer = build_optimizer(model, optim_cfg)          # OptimWrapper over torch's Adam, or FusedAdamOneCycle when
                                                           # optim_cfg.get('FNP_FUSED_STEP', False) is set
    lr_scheduler, _ = build_scheduler(optimizer, iters_per_epoch, epochs, last_epoch, optim_cfg)

SGD, plain Adam and adam_cosineanneal are not part of this library."""
from functools import partial

import torch.nn as nn
import torch.optim as optim

from .fastai_optim import OptimWrapper, bn_types
from .fused_adam_onecycle import FusedAdamOneCycle, LossScaler
from .learning_schedules_fastai import OneCycle

__all__ = ["build_optimizer", "build_scheduler", "OptimWrapper", "OneCycle", "FusedAdamOneCycle", "LossScaler", "layer_group_params"]


def _get(cfg, key, *default):
    if isinstance(cfg, dict):
        if key in cfg:
            return cfg[key]
    elif hasattr(cfg, key):
        return getattr(cfg, key)
    if default:
        return default[0]
    raise KeyError(key)


def _leaves(module):
    kids = list(module.children())
    if not kids:
        return [module]
    out = []
    for kid in kids:
        out += _leaves(kid)
    return out


def layer_group_params(model):
    """The two parameter lists the reference's adam_onecycle optimizer steps, in its order: the model's leaf modules in
    traversal order form one layer group, split into the non-BatchNorm leaves and the BatchNorm leaves; of each the trainable
    parameters, each once.  (A parameter held directly by a module that has children is in neither list, as in the reference.)"""
    groups = ([], [])
    seen = (set(), set())
    for leaf in _leaves(model):
        which = 1 if isinstance(leaf, bn_types) else 0
        for p in leaf.parameters():
            if p.requires_grad and id(p) not in seen[which]:
                seen[which].add(id(p))
                groups[which].append(p)
    return groups


def build_optimizer(model, optim_cfg):
    if _get(optim_cfg, "OPTIMIZER") != "adam_onecycle":
        raise NotImplementedError("only the adam_onecycle recipe is built here")
    betas = tuple(_get(optim_cfg, "BETAS", (0.9, 0.99)))
    wd = _get(optim_cfg, "WEIGHT_DECAY")
    if _get(optim_cfg, "FNP_FUSED_STEP", False):
        return FusedAdamOneCycle(layer_group_params(model), lr=3e-3, wd=wd, betas=betas)
    layer_groups = [nn.Sequential(*_leaves(model))]
    return OptimWrapper.create(partial(optim.Adam, betas=betas), 3e-3, layer_groups, wd=wd, true_wd=True, bn_wd=True)


def build_scheduler(optimizer, total_iters_each_epoch, total_epochs, last_epoch, optim_cfg):
    if _get(optim_cfg, "OPTIMIZER") != "adam_onecycle":
        raise NotImplementedError("only the adam_onecycle recipe is built here")
    total_steps = total_iters_each_epoch * total_epochs
    lr_scheduler = OneCycle(optimizer, total_steps, _get(optim_cfg, "LR"), list(_get(optim_cfg, "MOMS")),
                            _get(optim_cfg, "DIV_FACTOR"), _get(optim_cfg, "PCT_START"))
    return lr_scheduler, None
