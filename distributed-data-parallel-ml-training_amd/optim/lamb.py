"""LAMB: layer-wise trust ratios on the AdamW update (You et al. 2020) inside the fused update launch.

What LARS (optim/lars.py) is to SGD at the learning rates of a large global batch, LAMB is to
AdamW: every adapted tensor's update is scaled to the size of the tensor itself. The kernels
(csrc/kernels/optim.hip ``lamb_norms_kernel`` and the LAMB instantiations of ``sgd_pack_kernel``;
api.h LambArgs, LambNorms), the CPU path and the tests' oracle take the rule operation for
operation, all fp32, ``fma`` = one rounding, ``gs`` = ``grad_scale`` (times the clip coefficient
under the gradient guard), ``{a1, a2}`` = AdamW's bias-table entry of step ``t = lr_step + 1``:

    G   = g * gs
    m'  = fma(omb1, G - m, m)
    v'  = fma(omb2 * G, G, beta2 * v)
    den = fma(sqrt(v'), a2, eps)
    u   = m' / den                                  (so far AdamW, bit for bit)
    r   = fma(wd, p, a1 * u)                        the update direction, weight decay inside
    wn  = sqrt(sum p^2),  rn = sqrt(sum r^2)        over the tensor's own elements, p BEFORE the update
    trust = wn / rn   if the tensor is adapted and wn > 0 and rn > 0,   else 1.0
    p'  = fma(-(lr * trust), r, p)                  -(lr * trust): one fp32 product

A tensor is adapted when ``p.dim() > 1 or not exclude_1d`` (LARS's convention: biases and
BatchNorm vectors get 1.0); weight decay stays on for every tensor unless the ``no_decay`` mask
of FusedSGD takes it off (``"1d"`` or an iterable of parameters: ``r = fma(0, p, a1 u)`` for a
masked tensor, in both passes — bit 0 of the fourth field of its norms items and bit 8 of the
kind word of its update items select ``wd = 0`` for the block). LAMB has one rule for every
tensor, so a tensor with trust 1.0 is NOT bitwise AdamW: ``r`` folds the decay into the
direction, AdamW applies it to p first. There is no trust coefficient, no clamp of ``wn`` and no
per-group decay value or learning rate.

GPU: the ratio needs the norm of the update direction of a whole tensor before any element of it
moves, so an update takes two launches, both captured with the step. ``lamb_norms_kernel`` runs
one block per 8192-element chunk of the adapted tensors in the range, forms m', v', u and r in
registers, stores none of them and writes {sum p^2, sum r^2} into the slot of the chunk's number
in the WHOLE arena; the update launch sums its tensor's partials in a fixed order in every
block's prologue and forms the same r again from one shared device function. No float atomics,
no host sync. Launch order with the gradient guard: sum of squares, LAMB norms (which take the
clip coefficient from the guard's partials themselves: r is not linear in it), the update. A
step the guard skips uses no ratio and leaves the stored ones as they are. The partial, ratio
and table buffers are allocated once (the tables of LARS: optim/trust.py).

It refuses what its two parents refuse: no update in the backward, no ``step_elements``, no
sharded update; ``update="allreduce"`` is the plan. It composes with schedules, the guard (clip
first, then the norms of the clipped update), accumulation (one ratio per optimizer step, from
the averaged gradient), the weight EMA, soft targets and every gradient-sync strategy.

``state_dict`` has AdamW's layout plus ``exclude_1d`` in the group; a ``torch.optim.AdamW``
state dict loads.
"""
import torch

from .adamw import AdamW, _f32
from .sgd import fma32
from .trust import TrustTables


class LAMB(TrustTables, AdamW):
    _rule_launch_only = "LAMB's update rule exists in the step's own update launch only"
    metrics_name = "lamb"  # the ``optimizer`` field of --metrics records

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 grad_scale=1.0, max_grad_norm=None, clip_eps=1e-6, skip_nonfinite=False,
                 exclude_1d=True, no_decay=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                         grad_scale=grad_scale, max_grad_norm=max_grad_norm, clip_eps=clip_eps,
                         skip_nonfinite=skip_nonfinite, no_decay=no_decay)
        self.defaults["exclude_1d"] = bool(exclude_1d)
        self.param_groups[0]["exclude_1d"] = bool(exclude_1d)
        self._alloc_trust_tables()

    # ---------------------------------------------------------------------------------- step
    @torch.no_grad()
    def _cpu_step(self, params, c=None):
        """The module docstring's sequence on fp32 tensors; ``c``: the guard's clip coefficient
        (fp32 tensor) or None. The two sums are taken in fp64 and rounded once to fp32 (the
        oracle of the kernels' fp32 sums, as the guard's norm on the CPU)."""
        g = self.param_groups[0]
        f = lambda x: torch.tensor(float(x), dtype=torch.float32)  # noqa: E731
        lr = f(self._cpu_lr())
        a1, a2 = self.bias_at(self._lr_step)
        b1, b2 = g["betas"]
        omb1, beta2, omb2 = _f32(1.0 - b1), f(b2), f(1.0 - b2)
        gs = f(self._grad_scale_factor)
        if c is not None:
            gs = gs * c
        plist, adapted, trust = g["params"], self._adapted(), self.trust_ratios()
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
            r = fma32(_f32(self._wd_of(i)), p.float(), f(a1) * u)
            t = torch.ones((), dtype=torch.float32)
            if adapted[i]:
                wn = p.double().pow(2).sum().float().sqrt()
                rn = r.double().pow(2).sum().float().sqrt()
                if wn > 0 and rn > 0:
                    t = wn / rn
            trust[i] = t
            p.copy_(fma32(float(-(lr * t)), r, p.float()))

    @torch.no_grad()
    def step(self, closure=None, zero_grad=False, counter=None, skip=None, params=None,
             stream=None, fused_taken=False, signal=None, lr_advance=None, norm_done=False):
        """AdamW.step with the trust ratios: one norms launch over the adapted tensors of the
        range in front of the update launch (same arguments, same captured behaviour; with the
        gradient guard the sum-of-squares launch comes first, ``norm_done`` as in FusedSGD)."""
        if not self._fused or fused_taken:
            return super().step(closure, zero_grad=zero_grad, counter=counter, skip=skip,
                                params=params, stream=stream, fused_taken=fused_taken,
                                signal=signal, lr_advance=lr_advance, norm_done=norm_done)
        if lr_advance is None:
            lr_advance = params is None
        from ..ops.common import native, stream_handle
        s = stream.cuda_stream if stream is not None else stream_handle()
        a = self.arena
        rng = tuple(params) if params is not None else (0, len(a.params))
        items, n_items, descs = self._work_table(params)
        tables = self._trust_kw("lamb", rng)
        nitems, n_norm = self._norm_table(rng)
        if self.guarded and not norm_done:
            self.grad_sumsq(params, stream)
        adam = self._adam_kw()
        if n_norm:
            clip = {k: v for k, v in self._clip_kw(False).items() if k != "clip_stats"}
            native().lamb_norms(nitems.data_ptr(), n_norm, a.data.data_ptr(), a.grad.data_ptr(),
                                self.momentum_buffer.data_ptr(),
                                float(self.param_groups[0]["weight_decay"]),
                                float(self._grad_scale_factor), self._trust_partial.data_ptr(), s,
                                sched=self._sched_ptr(), **adam, **clip)
        self._update_launch(items, n_items, s, descs=descs, zero_grad=zero_grad, counter=counter,
                            skip=skip, signal=signal, lr_advance=lr_advance, **adam, **tables)
        return None

    # ----------------------------------------------------------------------------- checkpoints
    def load_state_dict(self, sd):
        saved = sd["param_groups"][0] if sd.get("param_groups") else {}
        ex = bool(saved.get("exclude_1d", self.param_groups[0]["exclude_1d"]))
        out = super().load_state_dict(sd)
        self.param_groups[0]["exclude_1d"] = ex
        return out
