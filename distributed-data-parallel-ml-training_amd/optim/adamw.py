"""AdamW: Adam with decoupled weight decay (Loshchilov & Hutter 2019) inside the fused update launch.

``torch.optim.AdamW`` with ``amsgrad=False``: decoupled decay ``p *= 1 - lr wd``, then
``p -= (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)`` with ``bc1 = 1 - beta1^t``,
``bc2 = 1 - beta2^t``. The kernel (csrc/kernels/optim.hip, the ADAM instantiations of
``sgd_pack_kernel``; api.h AdamArgs), the CPU path and the tests' oracle take it operation for
operation, all fp32, ``fma`` = one rounding, ``gs`` = ``grad_scale`` (times the clip coefficient
under the gradient guard):

    G   = g * gs
    m'  = fma(omb1, G - m, m)                      omb1 = float32(1 - beta1)   (lerp form)
    v'  = fma(omb2 * G, G, beta2 * v)              omb2 = float32(1 - beta2)
    den = fma(sqrt(v'), a2, eps)                   a2 = float32(1 / sqrt(1 - beta2^t))
    u   = m' / den
    p'  = fma(-(lr * a1), u, fma(-(lr * wd), p, p))    a1 = float32(1 / (1 - beta1^t))

``m`` lives in the momentum arena of FusedSGD (zero-initialised), ``v`` in one more fp32 arena
with the masters' element index, allocated once (captured graphs keep its address). The masters,
the gradient clear, the weight EMA and the bf16 operand re-pack stay in the one launch they were
in: AdamW changes the per-element rule, nothing around it.

The step number t inside a replayed graph: a hipGraph bakes float arguments in, so ``a1`` and
``a2`` are READ, like a scheduled learning rate, from a device table of ``{a1, a2}`` per step
(``bias_table``: computed in fp64, rounded once, entry k for t = k + 1, cut at the first entry
where both are exactly 1.0f; the kernel and the CPU path clamp the index to the last entry).
The index is the learning-rate schedule's step word (api.h LrSched: never written by a launch
that reads it), ``t = lr_step + 1``, so AdamW always owns a schedule: with none attached it
attaches a constant one (its learning rate is ``param_groups[0]["lr"]`` at that moment; call
``set_schedule(None)`` again after changing it), and ``set_schedule(None)`` re-attaches the
constant one and keeps the counter. Consequences: a step the gradient guard skipped still
advances t, because it advances the schedule (m, v, p and the EMA stay; the CPU path does the
same); an accumulated step (K micro-batches) advances t once; in the pipelined DDP step every
bucket's launch reads the same step and the last bucket stages the next.

The rule exists in the step's own update launch only (``updates_in_launch_only``): no update in
the backward, no ``step_elements``, no sharded update; ``update="allreduce"`` is the plan, as for
LARS and the EMA. It composes with schedules, the gradient guard, accumulation, the EMA, soft
targets and every gradient-sync strategy.

``no_decay`` (FusedSGD's per-tensor mask, ``"1d"`` or an iterable of parameters): a masked
tensor takes the rule with ``wd = 0``; ``-(lr * 0) = -0`` and ``fma(-0, p, p) = p``, so it is
``torch.optim.AdamW`` with a ``weight_decay=0`` group, bit for bit in ``p``. The update launch
takes the decision per work item (bit 8 of the kind word), once per block, in front of the
``-(lr * wd)`` product. Per-group decay VALUES and learning rates are not covered.

``state_dict`` uses torch.optim.AdamW's per-parameter layout ``{"step", "exp_avg",
"exp_avg_sq"}`` with ``step`` = ``lr_step``; a state dict written by torch.optim.AdamW for the
same parameters loads.
"""
import numpy as np
import torch

from .schedule import LRSchedule
from .sgd import FusedSGD, fma32

MAX_BIAS_ENTRIES = 1 << 20


def bias_table(beta1, beta2):
    """float32 [n][2] of {a1, a2} = {1 / (1 - beta1^t), 1 / sqrt(1 - beta2^t)}, entry k for
    t = k + 1: fp64, rounded once; cut after the first entry where both round to exactly 1.0f
    (every later step reads that entry). A beta that would need more than 2^20 entries is
    refused."""
    b1, b2 = float(beta1), float(beta2)
    chunks, k0, step = [], 0, 1 << 14
    while k0 < MAX_BIAS_ENTRIES:
        t = np.arange(k0 + 1, min(k0 + step, MAX_BIAS_ENTRIES) + 1, dtype=np.float64)
        a = np.stack([1.0 / (1.0 - np.power(b1, t)), 1.0 / np.sqrt(1.0 - np.power(b2, t))],
                     axis=1).astype(np.float32)
        one = np.nonzero((a[:, 0] == 1.0) & (a[:, 1] == 1.0))[0]
        if one.size:
            chunks.append(a[:one[0] + 1])
            return np.ascontiguousarray(np.concatenate(chunks))
        chunks.append(a)
        k0 += t.size
    last = chunks[-1][-1]
    name, b = ("beta1", b1) if last[0] != 1.0 else ("beta2", b2)
    raise ValueError(f"{name} = {b!r}: its bias correction is still not 1 after "
                     f"{MAX_BIAS_ENTRIES} steps; the device table holds at most 2^20 entries")


def _f32(x):
    return float(np.float32(x))


class AdamW(FusedSGD):
    _rule_launch_only = "AdamW's update rule exists in the step's own update launch only"
    metrics_name = "adamw"  # the ``optimizer`` field of --metrics records

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 grad_scale=1.0, max_grad_norm=None, clip_eps=1e-6, skip_nonfinite=False,
                 no_decay=None):
        self._check_hyper(betas, eps)
        if not float(lr) >= 0.0:
            raise ValueError("lr must be >= 0")
        if not float(weight_decay) >= 0.0:
            raise ValueError("weight_decay must be >= 0")
        table = bias_table(*betas)  # (refuses an unreasonable beta before anything is allocated)
        super().__init__(params, lr=lr, momentum=0.0, weight_decay=weight_decay,
                         grad_scale=grad_scale, max_grad_norm=max_grad_norm, clip_eps=clip_eps,
                         skip_nonfinite=skip_nonfinite, no_decay=no_decay)
        if len(self.param_groups) != 1:
            raise ValueError("AdamW supports a single param group")
        self._bias_dev = None
        self._set_hyper(betas, eps, table)
        if self._fused:
            # the first moment is FusedSGD's momentum arena; allocated once: captured launches
            # keep these addresses
            self.second_moment = torch.zeros_like(self.arena.data)
        self.set_schedule(None)

    @staticmethod
    def _check_hyper(betas, eps):
        b1, b2 = (float(b) for b in betas)
        if not 0.0 <= b1 < 1.0:
            raise ValueError(f"beta1 = {b1!r} must be in [0, 1)")
        if not 0.0 <= b2 < 1.0:
            raise ValueError(f"beta2 = {b2!r} must be in [0, 1)")
        if not float(eps) >= 0.0:
            raise ValueError("eps must be >= 0")

    def _set_hyper(self, betas, eps, table=None):
        """betas and eps into ``param_groups[0]`` and the bias table they give (constructor,
        load_state_dict). GPU: a table of another length is a new allocation: capture after."""
        self._check_hyper(betas, eps)
        hyper = {"betas": (float(betas[0]), float(betas[1])), "eps": float(eps), "amsgrad": False}
        self.defaults.update(hyper)
        self.param_groups[0].update(hyper)
        self._bias = table if table is not None else bias_table(*hyper["betas"])
        if self._fused:
            t = torch.from_numpy(self._bias).to(self.arena.data.device)
            if self._bias_dev is not None and self._bias_dev.shape == t.shape:
                self._bias_dev.copy_(t)
            else:
                self._bias_dev = t

    @property
    def bias(self):
        """The bias-correction table, float32 [n][2] on the host (do not modify)."""
        return self._bias

    def bias_at(self, k):
        """{a1, a2} of step index k (t = k + 1), the fp32 values every update uses."""
        a = self._bias[min(max(int(k), 0), len(self._bias) - 1)]
        return float(a[0]), float(a[1])

    def _state_arenas(self):
        return [self.momentum_buffer, self.second_moment]

    # ----------------------------------------------------------------------------- schedule
    def set_schedule(self, schedule, step=None):
        """As FusedSGD.set_schedule, but AdamW always owns a device schedule, whose step word
        numbers its steps: ``None`` (re-)attaches a constant one at the current learning rate
        and keeps the counter unless ``step`` is given."""
        if schedule is None:
            schedule = LRSchedule(float(self.param_groups[0]["lr"]), 1)
            step = self._lr_step if step is None else step
            self._own_schedule = True
        else:
            self._own_schedule = False
        super().set_schedule(schedule, step=0 if step is None else step)

    def _adam_kw(self):
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        return {"adam_v": self.second_moment.data_ptr(), "adam_bias": self._bias_dev.data_ptr(),
                "adam_n_bias": int(self._bias_dev.shape[0]), "adam_omb1": _f32(1.0 - b1),
                "adam_beta2": _f32(b2), "adam_omb2": _f32(1.0 - b2), "adam_eps": _f32(g["eps"])}

    # ---------------------------------------------------------------------------------- step
    @torch.no_grad()
    def _cpu_step(self, params, c=None):
        """The module docstring's sequence on fp32 tensors; ``c``: the guard's clip coefficient
        (fp32 tensor) or None."""
        g = self.param_groups[0]
        f = lambda x: torch.tensor(float(x), dtype=torch.float32)  # noqa: E731
        lr = f(self._cpu_lr())
        a1, a2 = self.bias_at(self._lr_step)
        b1, b2 = g["betas"]
        omb1, beta2, omb2 = _f32(1.0 - b1), f(b2), f(1.0 - b2)
        gs = f(self._grad_scale_factor)
        if c is not None:
            gs = gs * c
        nla = float(-(lr * f(a1)))
        plist = g["params"]
        for i in range(*(params if params is not None else (0, len(plist)))):
            p = plist[i]
            if p.grad is None:
                continue
            st = self.state[p]
            if "exp_avg" not in st:
                st["step"] = torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p, dtype=torch.float32)
                st["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32)
            m, v = st["exp_avg"], st["exp_avg_sq"]
            G = p.grad.float() * gs
            m.copy_(fma32(omb1, G - m, m))
            v.copy_(fma32(omb2 * G, G, beta2 * v))
            den = fma32(a2, v.sqrt(), torch.full_like(v, _f32(g["eps"])))
            u = m / den
            nlw = float(-(lr * f(self._wd_of(i))))  # (-0 under the no-decay mask: p stays)
            p.copy_(fma32(nla, u, fma32(nlw, p.float(), p.float())))

    @torch.no_grad()
    def step(self, closure=None, zero_grad=False, counter=None, skip=None, params=None,
             stream=None, fused_taken=False, signal=None, lr_advance=None, norm_done=False):
        """FusedSGD.step with the AdamW rule (same arguments, same captured behaviour). A step
        the guard skips changes no p, m, v or EMA and still counts: t follows the schedule."""
        if fused_taken:
            raise RuntimeError(self.launch_only_reason + ": no update is taken in the backward "
                               "(fused_taken)")
        if lr_advance is None:
            lr_advance = params is None
        if not self._fused:
            out = None
            if closure is not None:
                with torch.enable_grad():
                    out = closure()
            c, skipped = self._cpu_guard(lr_advance) if self.guarded else (None, False)
            if skipped:
                self._cpu_lr()
            else:
                self._cpu_step(params, c)
                self._cpu_ema(params)
            if lr_advance:
                self.count_step()
            if zero_grad:
                self.zero_grad()
            return out
        from ..ops.common import stream_handle
        s = stream.cuda_stream if stream is not None else stream_handle()
        items, n_items, descs = self._work_table(params)
        if self.guarded and not norm_done:
            self.grad_sumsq(params, stream)
        self._update_launch(items, n_items, s, descs=descs, zero_grad=zero_grad, counter=counter,
                            skip=skip, signal=signal, lr_advance=lr_advance, **self._adam_kw())
        return None

    # ----------------------------------------------------------------------------- checkpoints
    def state_dict(self):
        sd = super().state_dict()
        step = torch.tensor(float(self._lr_step))
        if self._fused:
            a = self.arena
            for i in range(len(a.params)):
                sd["state"][i] = {"step": step.clone(),
                                  "exp_avg": a.shaped(self.momentum_buffer, i).contiguous(),
                                  "exp_avg_sq": a.shaped(self.second_moment, i).contiguous()}
        else:
            for st in sd["state"].values():
                st["step"] = step.clone()
        return sd

    def load_state_dict(self, sd):
        saved = sd["param_groups"][0] if sd.get("param_groups") else {}
        st = sd.get("state", {})
        out = super().load_state_dict(sd)
        g = self.param_groups[0]
        g.setdefault("momentum", 0.0)  # (torch.optim.AdamW's groups have none)
        g.setdefault("nesterov", False)
        betas, eps = saved.get("betas", self.defaults["betas"]), saved.get("eps", self.defaults["eps"])
        if tuple(float(b) for b in betas) != self.defaults["betas"] or \
                float(eps) != self.defaults["eps"] or g.get("betas") != self.defaults["betas"]:
            self._set_hyper(betas, eps)
        g["betas"], g["eps"], g["amsgrad"] = self.defaults["betas"], self.defaults["eps"], False
        if saved.get("amsgrad", False):
            raise ValueError("amsgrad is not supported")
        if self._fused:
            a = self.arena
            for i, p in enumerate(a.params):
                e = st.get(i, st.get(str(i), {}))
                if e.get("exp_avg") is not None:
                    a.shaped(self.momentum_buffer, i).copy_(e["exp_avg"].reshape(p.shape))
                if e.get("exp_avg_sq") is not None:
                    a.shaped(self.second_moment, i).copy_(e["exp_avg_sq"].reshape(p.shape))
        if sd.get("lr_schedule") is None:
            # a state dict of torch.optim.AdamW: t is its per-parameter step; the constant
            # schedule takes the loaded learning rate
            steps = [int(float(e["step"])) for e in st.values() if "step" in e]
            self.set_schedule(None if self._own_schedule else self._schedule,
                              step=max(steps) if steps else self._lr_step)
        return out
