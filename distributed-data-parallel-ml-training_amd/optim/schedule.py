"""Per-step learning-rate schedule as one fp32 table.

The fast path replays a captured hipGraph, which bakes every float kernel argument in: a
learning rate that changes per step has to live in device memory (csrc/kernels/api.h LrSched,
uploaded by ``FusedSGD.set_schedule``). ``LRSchedule.table()`` is the single source of truth for
both sides: every entry is a closed form evaluated in float64 and rounded ONCE to fp32, the GPU
kernels read that fp32 value, and the CPU oracle sets ``param_groups[0]["lr"]`` to the same
value, so CPU and GPU train with bit-identical learning rates.

    k <  warmup_steps : base_lr * (f + (1 - f) * k / warmup_steps),  f = warmup_start_factor
    k >= warmup_steps : decay over j = k - warmup_steps of T = total_steps - warmup_steps steps
        constant : base_lr
        cosine   : min_lr + (base_lr - min_lr) * (1 + cos(pi * j / T)) / 2
        linear   : base_lr + (min_lr - base_lr) * j / T
        step     : base_lr * gamma ** #{m in milestones : m <= k}   (milestones in global steps)
    k >= total_steps  : the last entry (clamp)

These are torch.optim.lr_scheduler's LinearLR / CosineAnnealingLR(T_max=T, eta_min=min_lr) /
LinearLR(end_factor=min_lr/base_lr, total_iters=T) / MultiStepLR values in closed form.
"""
import math

import numpy as np
import torch

DECAYS = ("constant", "cosine", "linear", "step")


class LRSchedule:
    def __init__(self, base_lr, total_steps, warmup_steps=0, warmup_start_factor=0.0,
                 decay="constant", milestones=(), gamma=0.1, min_lr=0.0):
        if decay not in DECAYS:
            raise ValueError(f"decay must be one of {DECAYS}, got {decay!r}")
        if int(total_steps) < 1:
            raise ValueError("total_steps must be >= 1")
        if not 0 <= int(warmup_steps) <= int(total_steps):
            raise ValueError("warmup_steps must lie in [0, total_steps]")
        self.base_lr = float(base_lr)
        self.total_steps = int(total_steps)
        self.warmup_steps = int(warmup_steps)
        self.warmup_start_factor = float(warmup_start_factor)
        self.decay = decay
        self.milestones = sorted(int(m) for m in milestones)
        self.gamma = float(gamma)
        self.min_lr = float(min_lr)
        self._table = None

    def _lr64(self, k):
        b, w = self.base_lr, self.warmup_steps
        if k < w:
            f = self.warmup_start_factor
            return b * (f + (1.0 - f) * k / w)
        j, T = k - w, self.total_steps - w
        if self.decay == "cosine":
            return self.min_lr + (b - self.min_lr) * (1.0 + math.cos(math.pi * j / T)) / 2.0
        if self.decay == "linear":
            return b + (self.min_lr - b) * j / T
        if self.decay == "step":
            return b * self.gamma ** sum(1 for m in self.milestones if m <= k)
        return b

    def lr_at(self, k):
        """Learning rate of step k (0-based) as the fp32 value every update uses."""
        k = min(max(int(k), 0), self.total_steps - 1)
        return float(np.float32(self._lr64(k)))

    def table(self):
        """fp32 tensor of all ``total_steps`` learning rates (cached; do not modify)."""
        if self._table is None:
            vals = np.array([self._lr64(k) for k in range(self.total_steps)], dtype=np.float64)
            self._table = torch.from_numpy(vals.astype(np.float32))
        return self._table

    def state_dict(self):
        """Plain ints, floats and lists only (checkpoints load with weights_only=True)."""
        return {"base_lr": self.base_lr, "total_steps": self.total_steps,
                "warmup_steps": self.warmup_steps,
                "warmup_start_factor": self.warmup_start_factor, "decay": self.decay,
                "milestones": list(self.milestones), "gamma": self.gamma, "min_lr": self.min_lr}

    def load_state_dict(self, sd):
        self.__init__(**{k: sd[k] for k in self.state_dict()})
        return self

    @classmethod
    def from_state_dict(cls, sd):
        return cls(sd["base_lr"], sd["total_steps"]).load_state_dict(sd)

    def __repr__(self):
        return f"LRSchedule({self.state_dict()})"
