"""OptimWrapper for the adam_onecycle recipe: torch's Adam with the hyper-parameters as attributes that a schedule assigns every
iteration, and with decoupled weight decay.

What the recipe needs of it, and all that is here:
  * OptimWrapper.create(opt_func, lr, layer_groups, wd=..., true_wd=True, bn_wd=True), as the reference's build_optimizer calls it:
    every layer group becomes two parameter groups of the inner optimizer, first the trainable parameters of its non-BatchNorm
    children, then those of its BatchNorm children, so a state_dict lists the parameters in the reference's order;
  * `lr`, `mom` (Adam's beta1), `beta` (beta2) and `wd` read and assigned as plain numbers: OneCycle assigns lr and mom every step;
  * step(): with true_wd every trainable parameter is multiplied by 1 - wd * lr, with a gradient or without (BatchNorm
    parameters too unless bn_wd is off), and Adam then steps with its own weight_decay at 0; without true_wd, wd is Adam's own
    weight_decay (L2) and step() is Adam's;
  * everything else (param_groups, state_dict, load_state_dict, ... : what GradScaler and a checkpoint ask for) is the inner
    optimizer's.
Optimizers without `betas`, per-layer-group learning rates and the reference's mixed-precision master copies are not part of it."""
from torch import nn

bn_types = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d, nn.SyncBatchNorm)


def _number(val):
    """a schedule may hand over a one-element list or a numpy scalar"""
    if isinstance(val, (list, tuple)):
        assert len(set(val)) == 1, "one value for all layer groups"
        val = val[0]
    return float(val)


class OptimWrapper:
    def __init__(self, opt, wd, true_wd=False, bn_wd=True):
        first = opt.param_groups[0]
        assert "betas" in first and len(opt.param_groups) % 2 == 0, "an Adam-like optimizer over (non-BatchNorm, BatchNorm) pairs of groups"
        self.opt, self.true_wd, self.bn_wd = opt, bool(true_wd), bool(bn_wd)
        self._hyper = {"lr": float(first["lr"]), "mom": float(first["betas"][0]), "beta": float(first["betas"][1]), "wd": _number(wd)}
        self._write()

    @classmethod
    def create(cls, opt_func, lr, layer_groups, **kwargs):
        groups = []
        for layer_group in layer_groups:
            halves = ([], [])
            for child in layer_group.children():
                halves[isinstance(child, bn_types)].append(child)
            for half in halves:
                seen, params = set(), []
                for child in half:
                    for p in child.parameters():
                        if p.requires_grad and id(p) not in seen:
                            seen.add(id(p))
                            params.append(p)
                groups.append({"params": params, "lr": 0})
        wrapper = cls(opt_func(groups), **kwargs)
        wrapper.lr = lr
        return wrapper

    def _write(self):
        """the hyper-parameters into the inner optimizer's groups (odd groups hold the BatchNorm parameters)"""
        h = self._hyper
        for i, group in enumerate(self.opt.param_groups):
            group["lr"], group["betas"] = h["lr"], (h["mom"], h["beta"])
            group["weight_decay"] = 0 if self.true_wd or (i % 2 == 1 and not self.bn_wd) else h["wd"]

    def _assign(self, name, val):
        if val is not None:
            self._hyper[name] = _number(val)
            self._write()

    lr = property(lambda self: self._hyper["lr"], lambda self, val: self._assign("lr", val))
    mom = property(lambda self: self._hyper["mom"], lambda self, val: self._assign("mom", val))
    beta = property(lambda self: self._hyper["beta"], lambda self, val: self._assign("beta", val))
    wd = property(lambda self: self._hyper["wd"], lambda self, val: self._assign("wd", val))

    def step(self):
        if self.true_wd:
            factor = 1 - self._hyper["wd"] * self._hyper["lr"]
            for i, group in enumerate(self.opt.param_groups):
                if i % 2 == 0 or self.bn_wd:
                    for p in group["params"]:
                        if p.requires_grad:
                            p.data.mul_(factor)
        self.opt.step()

    def zero_grad(self):
        self.opt.zero_grad()

    def __getattr__(self, name):
        if name == "opt":           # (not set yet: unpickling, or a failed __init__)
            raise AttributeError(name)
        return getattr(self.opt, name)

    def __repr__(self):
        return f"OptimWrapper(true_wd={self.true_wd}, bn_wd={self.bn_wd}, {self._hyper}) over {self.opt!r}"
