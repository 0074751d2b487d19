"""Learning-rate schedules that a captured step can follow: a table on the device, indexed by the step counter.

`VariableManager.register(..., learning_rate=LRSchedule...)` makes Adam read its rate from the table: on the fused
path `p2l_adam_step_sched` takes `table[min(completed steps, len - 1)]` on the device, where the per-sample step
counters already live (a scalar launch argument would be baked into a captured HIP graph); on the generic path
(CPU tensors, another optimizer class) the closure sets each parameter group's 'lr' from `value(step)` before
`opt.step`.  The table is made on the host, in Python floats rounded once to fp32.

`projector_ramp` is the StyleGAN2 projector's schedule AS RECALLED -- UNPINNED: that file is not in the reference
tree, so the formula in its docstring is the definition here.
"""
import hashlib
import math

import numpy as np
import torch


class LRSchedule(object):
    """An fp32 table of learning rates, one per step; after its end the last value holds."""

    def __init__(self, values):
        v = np.asarray([float(x) for x in values], dtype=np.float64).astype(np.float32)
        if v.ndim != 1 or v.size < 1:
            raise ValueError('LRSchedule: a table of at least one learning rate, got %d' % v.size)
        if not np.isfinite(v).all():
            raise ValueError('LRSchedule: the table holds a value that is not finite')
        self.values = v
        self.values.setflags(write=False)
        self._digest = hashlib.sha1(v.tobytes()).hexdigest()
        self._on_device = {}

    # ---- constructors
    @classmethod
    def constant(cls, lr):
        return cls([lr])

    @classmethod
    def cosine(cls, lr, num_steps, final=0.0):
        """value_i = final + (lr - final) * (0.5 + 0.5 cos(pi i / (num_steps - 1))), i = 0 .. num_steps - 1: `lr` at
        the first step, `final` at the last and from there on"""
        n = int(num_steps)
        if n < 1:
            raise ValueError('LRSchedule.cosine: num_steps must be at least 1, got %d' % n)
        if n == 1:
            return cls([lr])
        vals = [final + (lr - final) * (0.5 + 0.5 * math.cos(math.pi * i / (n - 1))) for i in range(n)]
        vals[0], vals[-1] = lr, final                   # (the end points exactly)
        return cls(vals)

    @classmethod
    def projector_ramp(cls, lr, num_steps, rampdown=0.25, rampup=0.05):
        """The StyleGAN2 projector's schedule as recalled (UNPINNED; this formula is the definition): for
        i = 0 .. num_steps - 1
            t = i / num_steps;  r = min(1, (1 - t) / rampdown);  r = 0.5 - 0.5 cos(pi r);  r = r * min(1, t / rampup)
            value_i = lr * r
        a linear ramp up over the first `rampup` of the run, a cosine ramp down over the last `rampdown`."""
        n = int(num_steps)
        if n < 1:
            raise ValueError('LRSchedule.projector_ramp: num_steps must be at least 1, got %d' % n)
        vals = []
        for i in range(n):
            t = i / n
            r = min(1.0, (1.0 - t) / rampdown)
            r = 0.5 - 0.5 * math.cos(math.pi * r)
            r = r * min(1.0, t / rampup)
            vals.append(lr * r)
        return cls(vals)

    # ----
    def __len__(self):
        return int(self.values.size)

    def value(self, i):
        """the rate of the step after `i` completed ones, as a Python float (the fp32 table value)"""
        i = int(i)
        return float(self.values[min(max(i, 0), self.values.size - 1)])

    def graph_key(self):
        """what a captured step bakes in of this schedule (optimizer/base_optimizer.py `_graph_key`)"""
        return ('LRSchedule', self._digest)

    def device_table(self, device):
        """the table as an fp32 tensor on `device`, made once per device"""
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        t = self._on_device.get(device)
        if t is None:
            if device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
                raise RuntimeError('LRSchedule: first use on %s inside a graph capture; call it once eagerly' % device)
            t = self._on_device[device] = torch.from_numpy(self.values.copy()).to(device)
        return t

    def __repr__(self):
        return 'LRSchedule(%d values, first %g, last %g)' % (len(self), self.values[0], self.values[-1])
