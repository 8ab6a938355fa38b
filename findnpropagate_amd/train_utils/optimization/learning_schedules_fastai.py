"""The reference's OneCycle schedule (tools/train_utils/optimization/learning_schedules_fastai.py), restated: per iteration
it sets `optimizer.lr` and `optimizer.mom` (Adam's beta1) by cosine interpolation in two phases.

With a = int(total_step * pct_start):
    steps [0, a):            lr: lr_max / div_factor -> lr_max,            mom: moms[0] -> moms[1]
    steps [a, total_step):   lr: lr_max -> lr_max / div_factor / 1e4,      mom: moms[1] -> moms[0]
each as  end + (start - end) / 2 * (cos(pi * pct) + 1)  at pct = (step - phase start) / (phase length)."""
import numpy as np


def annealing_cos(start, end, pct):
    """from `start` (pct 0) to `end` (pct 1) along half a cosine"""
    return end + (start - end) / 2 * (np.cos(np.pi * pct) + 1)


class LRSchedulerStep:
    """lr_phases / mom_phases: sequences of (start as a fraction of total_step, f(pct)); a phase runs to the start of the next"""

    def __init__(self, fai_optimizer, total_step, lr_phases, mom_phases):
        self.optimizer = fai_optimizer
        self.total_step = total_step
        self.lr_phases = self._spans(lr_phases, total_step)
        self.mom_phases = self._spans(mom_phases, total_step)

    @staticmethod
    def _spans(phases, total_step):
        starts = [int(start * total_step) for start, _ in phases]
        assert starts[0] == 0 and all(a < b for a, b in zip(starts, starts[1:]))
        ends = starts[1:] + [total_step]
        return [(s, e, f) for s, e, (_, f) in zip(starts, ends, phases)]

    def step(self, step, epoch=None):
        # the last phase that has begun decides (an earlier one is evaluated and overwritten in the reference)
        for attr, phases in (("lr", self.lr_phases), ("mom", self.mom_phases)):
            for start, end, f in phases:
                if step >= start:
                    setattr(self.optimizer, attr, f((step - start) / (end - start)))


class OneCycle(LRSchedulerStep):
    def __init__(self, fai_optimizer, total_step, lr_max, moms, div_factor, pct_start):
        self.lr_max, self.moms, self.div_factor, self.pct_start = lr_max, moms, div_factor, pct_start
        low_lr = lr_max / div_factor
        up = lambda a, b: (lambda pct: annealing_cos(a, b, pct))
        lr_phases = ((0, up(low_lr, lr_max)), (pct_start, up(lr_max, low_lr / 1e4)))
        mom_phases = ((0, up(moms[0], moms[1])), (pct_start, up(moms[1], moms[0])))
        fai_optimizer.lr, fai_optimizer.mom = low_lr, moms[0]
        super().__init__(fai_optimizer, total_step, lr_phases, mom_phases)
