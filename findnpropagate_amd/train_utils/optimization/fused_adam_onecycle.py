"""The optimizer span of the reference's adam_onecycle training loop as one device-resident step.

The reference's loop (tools/train_utils/train_utils.py:172-176):

    scaler.scale(loss).backward()
    scaler.unscale_(optimizer)                                   # a multi-tensor unscale, then a host read of found_inf
    clip_grad_norm_(model.parameters(), optim_cfg.GRAD_NORM_CLIP)
    scaler.step(optimizer)                                       # OptimWrapper.step: one mul_ per parameter, then Adam
    scaler.update()

with FusedAdamOneCycle and LossScaler:

    scaler.scale(loss).backward()
    optimizer.step_scaled(scaler, optim_cfg.GRAD_NORM_CLIP)      # fnp_adam_onecycle_step: three launches, no host read

The contract of the step is stated in include/fnp.h (fnp_adam_onecycle_step).  Two deviations from the reference's span: the
gradients are left as they came (scaled, unclipped; nothing reads them before the next zero_grad), and a non-finite gradient
skips the step also without a scaler (the reference would write NaN into the parameters).

FusedAdamOneCycle has OptimWrapper's properties (`lr`, `mom`, `beta`, `wd`), so the OneCycle schedule drives it unchanged, and
torch Adam's state_dict format, so a checkpoint of either loads into the other."""
import math

import numpy as np
import torch

from ... import lib

CHUNK = 8192      # elements per workgroup of the kernels (a multiple of 4); small tensors take one chunk each

_CHUNK_DTYPE = np.dtype([("tensor", "<i4"), ("length", "<i4"), ("offset", "<i8")])      # struct fnp_optim_chunk


def chunk_table(lengths, chunk=CHUNK):
    """struct fnp_optim_chunk per workgroup: every element of every tensor in exactly one chunk, in order"""
    assert chunk > 0 and chunk % 4 == 0
    rows = [(i, min(chunk, n - off), off) for i, n in enumerate(lengths) for off in range(0, n, chunk)]
    return np.array(rows, dtype=_CHUNK_DTYPE)


def _last(val):
    return val[-1] if isinstance(val, (list, tuple)) else val


class LossScaler:
    """torch's GradScaler with its state on the device and no host read: `scale(loss)` multiplies by the device-resident
    scale; FusedAdamOneCycle.step_scaled unscales, checks, steps and updates the scale in its own launches.  get_scale() is the
    only call that reads.  state_dict() carries GradScaler's keys."""

    def __init__(self, enabled=True, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        assert growth_factor > 1.0 and 0.0 < backoff_factor < 1.0 and growth_interval >= 1
        self._enabled = bool(enabled)
        self._init_scale, self._init_growth_tracker = float(init_scale), 0
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self._scale = self._growth_tracker = None

    def is_enabled(self):
        return self._enabled

    def tensors(self, device):
        """(scale, growth_tracker) on `device`, made at the first use (as GradScaler makes its own lazily)"""
        if self._scale is None or self._scale.device != torch.device(device):
            old = self._scale
            self._scale = torch.full((1,), self._init_scale, dtype=torch.float32, device=device) if old is None else old.to(device)
            self._growth_tracker = (torch.full((1,), self._init_growth_tracker, dtype=torch.int32, device=device)
                                    if old is None else self._growth_tracker.to(device))
        return self._scale, self._growth_tracker

    def scale(self, loss):
        if not self._enabled:
            return loss
        # the f32 scale as a 0-dim tensor, uncast, as GradScaler multiplies: a 0-dim half loss is promoted to f32 (2^16 is not a half)
        return loss * self.tensors(loss.device)[0].squeeze(0)

    def get_scale(self):
        if not self._enabled:
            return 1.0
        return self._init_scale if self._scale is None else float(self._scale.item())

    def state_dict(self):
        if not self._enabled:
            return {}
        return {"scale": self.get_scale(), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval,
                "_growth_tracker": self._init_growth_tracker if self._growth_tracker is None else int(self._growth_tracker.item())}

    def load_state_dict(self, state):
        if not self._enabled:
            return
        if not state:
            raise RuntimeError("the state comes from a disabled scaler")
        self._init_scale, self._init_growth_tracker = float(state["scale"]), int(state["_growth_tracker"])
        self.growth_factor, self.backoff_factor = float(state["growth_factor"]), float(state["backoff_factor"])
        self.growth_interval = int(state["growth_interval"])
        if self._scale is not None:
            self._scale.fill_(self._init_scale)
            self._growth_tracker.fill_(self._init_growth_tracker)


class FusedAdamOneCycle:
    """Adam with decoupled weight decay over two parameter groups (non-BatchNorm, BatchNorm: layer_group_params), stepped by
    fnp_adam_onecycle_step.  `params`: the two lists.  State per parameter: exp_avg, exp_avg_sq (f32 like the parameter) and a
    step count, all on the parameter's device; the counts live in one int32 tensor."""

    def __init__(self, params, lr=3e-3, wd=0.0, betas=(0.9, 0.99), eps=1e-8, chunk=CHUNK):
        groups = [list(g) for g in params]
        assert len(groups) == 2, "two parameter groups: non-BatchNorm, BatchNorm"
        self.group_sizes = [len(g) for g in groups]
        self.params = groups[0] + groups[1]
        assert len({id(p) for p in self.params}) == len(self.params), "a parameter appears twice"
        self.lr, self.mom, self.beta, self.wd, self.eps = lr, betas[0], betas[1], wd, float(eps)
        self.true_wd = self.bn_wd = True
        self.chunk = int(chunk)
        dev = self.params[0].device if self.params else torch.device("cpu")
        self.exp_avg = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.steps = torch.zeros((len(self.params),), dtype=torch.int32, device=dev)
        self.last_grad_norm = torch.zeros((1,), dtype=torch.float32, device=dev)
        self.last_found_inf = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.uploads = 0            # host-to-device copies of the pointer table so far
        self.fused_steps = 0        # steps the kernels took
        self._sent = None           # the pointer table as last uploaded (a tuple of addresses)
        self._traits = None         # (dtype, contiguity, length) of every gradient as last checked by fused_reasons
        self._table = self._pinned = self._chunks = self._workspace = self._consumed = None

    # ------------------------------------------------------------------------------------------ hyper-parameters
    lr = property(lambda self: self._lr, lambda self, val: setattr(self, "_lr", float(_last(val))))
    mom = property(lambda self: self._mom, lambda self, val: setattr(self, "_mom", float(_last(val))))
    beta = property(lambda self: self._beta, lambda self, val: val is None or setattr(self, "_beta", float(_last(val))))
    wd = property(lambda self: self._wd, lambda self, val: setattr(self, "_wd", float(_last(val))))

    @property
    def param_groups(self):
        """torch Adam's view of the two groups (read-only: the properties are the way to set a hyper-parameter)"""
        out, start = [], 0
        for size in self.group_sizes:
            group = dict(self._group_template(), lr=self._lr, betas=(self._mom, self._beta), eps=self.eps, weight_decay=0)
            group["params"] = self.params[start:start + size]
            out.append(group)
            start += size
        return out

    _template = None

    @classmethod
    def _group_template(cls):
        if cls._template is None:       # whatever keys this torch's Adam keeps in a group
            cls._template = {k: v for k, v in torch.optim.Adam([torch.zeros(0)]).param_groups[0].items() if k != "params"}
        return cls._template

    # ------------------------------------------------------------------------------------------ the routes
    def fused_reasons(self):
        """what stands against the kernels, as a list of short strings (empty: fnp_adam_onecycle_step runs); with a reason
        the plain torch route of the same contract runs instead"""
        r = []
        tensors = self.params + [p.grad for p in self.params if p.grad is not None]
        if any(not t.is_cuda for t in tensors):
            r.append("CPU tensors")
        if len({t.device for t in tensors} | {self.steps.device}) > 1:
            r.append("more than one device")
        if any(t.dtype != torch.float32 for t in tensors):
            r.append("a dtype other than f32")
        if any(not t.is_contiguous() for t in tensors):
            r.append("a non-contiguous parameter or gradient")
        if any(p.grad is not None and p.grad.shape != p.shape for p in self.params):
            r.append("a gradient of another shape")
        return r

    def zero_grad(self):
        """in place: the gradients keep their addresses, so the pointer table stays as uploaded"""
        grads = [p.grad for p in self.params if p.grad is not None]
        for g in grads:
            if g.grad_fn is not None:
                g.detach_()
            else:
                g.requires_grad_(False)
        if grads:
            torch._foreach_zero_(grads)

    def step(self):
        self.step_scaled(None, math.inf)

    def step_scaled(self, scaler=None, max_norm=math.inf):
        """unscale, non-finite check, clip to `max_norm`, decay, Adam, scale update: the contract of fnp_adam_onecycle_step"""
        if scaler is not None and not scaler.is_enabled():
            scaler = None
        max_norm = float(max_norm)
        if not self.params:
            return
        # (an empty gradient has no address: it is present all the same, and stands in the table as an address nothing reads)
        here = self.steps.data_ptr()
        grads = [p.grad for p in self.params]
        pointers = tuple(p.data_ptr() for p in self.params) + tuple(0 if g is None else g.data_ptr() or here for g in grads)
        # what the kernels take on trust of a gradient besides its address: a gradient rebound at the same address as another
        # dtype, a strided view or a shorter tensor must not be streamed as the one that was checked
        traits = tuple(None if g is None else (g.dtype, g.is_contiguous(), g.numel()) for g in grads)
        if pointers != self._sent or traits != self._traits:
            if self.fused_reasons():        # (checked when an address or a trait changed, not every step)
                return self._step_plain(scaler, max_norm)
            if pointers != self._sent:
                self._upload(pointers)
            self._traits = traits
        scale, tracker = scaler.tensors(self.steps.device) if scaler is not None else (None, None)
        n = len(self.params)
        L = lib.load()
        table = self._table.data_ptr()
        lib.check(L.fnp_adam_onecycle_step(
            n, int(self._chunks.shape[0]), lib.ptr(self._chunks), table, table + 8 * n, table + 16 * n, table + 24 * n,
            lib.ptr(self.steps), lib.ptr(scale), lib.ptr(tracker), self._lr, self._mom, self._beta, self.eps, self._wd, max_norm,
            scaler.growth_factor if scaler else 2.0, scaler.backoff_factor if scaler else 0.5, scaler.growth_interval if scaler else 1,
            lib.ptr(self._workspace), self._workspace.numel(), lib.ptr(self.last_grad_norm), lib.ptr(self.last_found_inf),
            lib.stream()), "fnp_adam_onecycle_step")
        self.fused_steps += 1

    def _upload(self, pointers):
        """the four pointer tables (params, grads, exp_avg, exp_avg_sq) to the device, asynchronously from pinned memory; the
        pinned buffer is rewritten only once the copy before has been consumed"""
        n, dev = len(self.params), self.steps.device
        if self._table is None:
            self._table = torch.zeros((4 * n,), dtype=torch.int64, device=dev)
            self._pinned = torch.zeros((4 * n,), dtype=torch.int64)
            if dev.type == "cuda":
                self._pinned = self._pinned.pin_memory()
                self._consumed = torch.cuda.Event()
            table = chunk_table([p.numel() for p in self.params], self.chunk)
            self._chunks = torch.from_numpy(table.view(np.uint8).reshape(table.shape[0], _CHUNK_DTYPE.itemsize)).to(dev)
            bytes_ = int(lib.load().fnp_adam_onecycle_workspace_bytes(int(table.shape[0])))
            self._workspace = torch.zeros(((bytes_ + 7) // 8,), dtype=torch.int64, device=dev).view(torch.uint8)
        elif self._consumed is not None:
            self._consumed.synchronize()
        host = self._pinned.numpy()
        host[:2 * n] = pointers
        host[2 * n:3 * n] = [t.data_ptr() for t in self.exp_avg]
        host[3 * n:] = [t.data_ptr() for t in self.exp_avg_sq]
        self._table.copy_(self._pinned, non_blocking=True)
        if self._consumed is not None:
            self._consumed.record()
        self._sent = pointers
        self.uploads += 1

    def _step_plain(self, scaler, max_norm):
        """the same contract in torch operations, in the parameters' own dtype (what runs on CPU tensors); it reads
        found_inf and the step counts on the host"""
        self._sent = self._traits = None
        dev = self.steps.device
        scale, tracker = scaler.tensors(dev) if scaler is not None else (None, None)
        inv = (1.0 / scale.double()).float() if scale is not None else torch.ones((1,), dtype=torch.float32, device=dev)
        with torch.no_grad():
            unscaled = [None if p.grad is None else p.grad * inv.to(p.grad.device) for p in self.params]
            total = torch.zeros((), dtype=torch.float64, device=dev)
            finite = True
            for g in unscaled:
                if g is not None:
                    total = total + (g.double() * g.double()).sum().to(dev)
                    finite = finite and bool(torch.isfinite(g).all())
            norm = total.sqrt()
            self.last_grad_norm = norm.float().reshape(1)
            self.last_found_inf = torch.full((1,), 0 if finite else 1, dtype=torch.int32, device=dev)
            if not finite:
                if scale is not None:
                    scale.mul_(scaler.backoff_factor)
                    tracker.zero_()
                return
            clip = min(1.0, max_norm / (float(norm) + 1e-6))
            counts = self.steps.tolist()
            for i, (p, g, m, v) in enumerate(zip(self.params, unscaled, self.exp_avg, self.exp_avg_sq)):
                p.mul_(1 - self._wd * self._lr)
                if g is None:
                    continue
                counts[i] += 1
                g = g * clip
                m.add_((g - m) * (1 - self._mom))
                v.mul_(self._beta).add_(((1 - self._beta) * g) * g)
                step_size = self._lr / (1 - self._mom ** counts[i])
                den = v.sqrt().div_(math.sqrt(1 - self._beta ** counts[i])).add_(self.eps)
                p.sub_(step_size * (m / den))
            self.steps.copy_(torch.tensor(counts, dtype=torch.int32))
            if scale is not None:
                ok = int(tracker.item()) + 1
                if ok == scaler.growth_interval:
                    grown = scale * scaler.growth_factor
                    if bool(torch.isfinite(grown).all()):
                        scale.copy_(grown)
                    ok = 0
                tracker.fill_(ok)

    # ------------------------------------------------------------------------------------------ torch Adam's state format
    def state_dict(self):
        counts = self.steps.tolist()
        state = {i: {"step": torch.tensor(float(t), dtype=torch.float32), "exp_avg": self.exp_avg[i], "exp_avg_sq": self.exp_avg_sq[i]}
                 for i, t in enumerate(counts) if t > 0}
        groups, start = [], 0
        for group, size in zip(self.param_groups, self.group_sizes):
            group["params"] = list(range(start, start + size))
            groups.append(group)
            start += size
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, state_dict):
        groups = state_dict["param_groups"]
        if [len(g["params"]) for g in groups] != self.group_sizes:
            raise ValueError("loaded state dict has other parameter groups")
        order = [i for g in groups for i in g["params"]]
        counts = [0] * len(self.params)
        with torch.no_grad():
            for k, (m, v) in enumerate(zip(self.exp_avg, self.exp_avg_sq)):
                entry = state_dict["state"].get(order[k])
                if entry is None:       # torch's Adam makes a parameter's state at its first gradient
                    m.zero_(); v.zero_()
                    continue
                counts[k] = int(round(float(entry["step"])))
                m.copy_(entry["exp_avg"].reshape(m.shape)); v.copy_(entry["exp_avg_sq"].reshape(v.shape))
            self.steps.copy_(torch.tensor(counts, dtype=torch.int32))
        last = groups[-1]
        self.lr, self.eps = last["lr"], float(last["eps"])
        self.mom, self.beta = last["betas"]
