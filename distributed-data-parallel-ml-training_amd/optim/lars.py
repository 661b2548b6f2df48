"""LARS: layer-wise adaptive rate scaling (You, Gitman, Ginsburg 2017) on top of the fused SGD.

Large-batch training multiplies the learning rate by the batch ratio (utils/cli.py
``--lr-ref-batch``); a conv net with BatchNorm tolerates that rate only when each tensor's update
is scaled to the size of the tensor itself. All arithmetic is fp32; ``gs`` = ``grad_scale``:

    adapted_i = p_i.dim() > 1 or not exclude_1d
    wn = sqrt(sum(p_i^2));  gn = sqrt(sum((g_i * gs)^2))          (the tensor's own elements)
    trust_i = eta * wn / (gn + wd * wn + eps)   if adapted_i and wn > 0 and gn > 0   else 1.0
    d   = trust_i * fma(wd, p, g * gs)
    buf = fma(momentum, buf, d);  d = nesterov ? fma(momentum, buf, d) : buf
    p   = fma(-lr, d, p)

A tensor whose ratio is 1.0 takes the plain SGD update bit for bit; weight decay stays on for
every tensor unless the ``no_decay`` mask of FusedSGD takes it off (``"1d"`` or an iterable of
parameters): a masked tensor runs with ``wd = 0`` in the update and, when it is adapted
(``exclude_1d=False``), in its ratio, ``eta * wn / (gn + eps)``. Conv masters are stored [K][R][S][C] on the GPU: a norm does not depend on the
element order.

GPU: two launches per update launch of FusedSGD, both captured with the step
(csrc/kernels/optim.hip): ``chunk_sums_kernel<true>`` writes one {sum p^2, sum (g gs)^2} partial
per 8192-element chunk of every adapted tensor in the range, into the slot of the chunk's number
in the WHOLE arena (per-bucket launches on the comm stream never share a slot), and the LARS
instantiation of ``sgd_pack_kernel`` (the fused SGD + re-pack) sums its tensor's partials in a
fixed order in every block's prologue. No float atomics, no host sync: the result is
reproducible and does not depend on the launch's parameter range. The partial and ratio buffers
are allocated once, so their addresses survive re-captures.

What LARS cannot do: an update that runs before the whole gradient exists (SGD in the backward)
or that sees only a shard of a tensor (ZeRO-1, the bf16-gather sharded update) has no norm to
use. Those paths refuse this optimizer; the all-reduce update (``update="allreduce"``) is the
one to use.

With the gradient guard of FusedSGD (``max_grad_norm``, ``skip_nonfinite``; optim/sgd.py): clip
first. The ratio takes c * gn as the gradient norm (sum (g gs c)^2 = c^2 sum (g gs)^2: no
second pass over the gradient) and the update runs with gs * c. Launch order: sum of squares,
LARS norms, the clipped LARS update.

With the weight EMA of FusedSGD (``set_ema``): the same launch advances the average from the
new master; nothing else changes (LARS already keeps every update in the step's launch).
"""
import torch

from .sgd import FusedSGD
from .trust import TrustTables

_SHARDED = ("LARS needs every tensor's whole gradient for its norm: the sharded updates split "
            "tensors across ranks; use the replicated update, update=\"allreduce\"")


class LARS(TrustTables, FusedSGD):
    def __init__(self, params, lr=0.1, momentum=0.0, dampening=0.0, weight_decay=0.0,
                 nesterov=False, grad_scale=1.0, trust_coefficient=0.001, eps=1e-8,
                 exclude_1d=True, max_grad_norm=None, clip_eps=1e-6, skip_nonfinite=False,
                 no_decay=None):
        if dampening != 0.0:
            raise ValueError("LARS supports dampening=0 only")
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening,
                         weight_decay=weight_decay, nesterov=nesterov, grad_scale=grad_scale,
                         max_grad_norm=max_grad_norm, clip_eps=clip_eps,
                         skip_nonfinite=skip_nonfinite, no_decay=no_decay)
        if len(self.param_groups) != 1:
            raise ValueError("LARS supports a single param group")
        hyper = {"trust_coefficient": float(trust_coefficient), "eps": float(eps),
                 "exclude_1d": bool(exclude_1d)}
        self.defaults.update(hyper)
        self.param_groups[0].update(hyper)
        self._alloc_trust_tables()

    # ------------------------------------------------------------------------------ refusals
    def register_in_backward(self):
        raise RuntimeError("LARS cannot run in the backward: a tensor's gradient norm exists "
                           "only once its whole gradient does (TrainStep keeps opt_in_bwd False)")

    def step_elements(self, lo, hi, **kw):
        raise ValueError(_SHARDED)

    # ---------------------------------------------------------------------------------- step
    @torch.no_grad()
    def _cpu_step(self, params, c=None):
        """``c``: the guard's clip coefficient (fp32 tensor) or None."""
        g = self.param_groups[0]
        lr = self._cpu_lr()
        m, nesterov = float(g["momentum"]), bool(g["nesterov"])
        eta, eps = float(g["trust_coefficient"]), float(g["eps"])
        gs = float(self._grad_scale_factor)
        plist, adapted, trust = g["params"], self._adapted(), self.trust_ratios()
        for i in range(*(params if params is not None else (0, len(plist)))):
            p = plist[i]
            if p.grad is None:
                continue
            wd = self._wd_of(i)
            gr = p.grad * gs
            if c is not None:  # clip first: the update runs with gs * c ...
                gr = p.grad * (torch.tensor(gs, dtype=torch.float32) * c)
            d = gr.add(p, alpha=wd)
            t = torch.ones((), dtype=torch.float32)
            if adapted[i]:
                wn, gn = p.pow(2).sum().sqrt(), (p.grad * gs).pow(2).sum().sqrt()
                if c is not None:  # ... and the ratio takes c * gn
                    gn = c * gn
                if wn > 0 and gn > 0:
                    t = eta * wn / (gn + wd * wn + eps)
            trust[i] = t
            d = d * t
            if m != 0:
                st = self.state[p]
                if "momentum_buffer" not in st:  # zero start == torch's first-step clone
                    st["momentum_buffer"] = torch.zeros_like(p)
                buf = st["momentum_buffer"]
                buf.mul_(m).add_(d)
                d = d.add(buf, alpha=m) if nesterov else buf
            p.add_(d, alpha=-lr)

    @torch.no_grad()
    def step(self, closure=None, zero_grad=False, counter=None, skip=None, params=None,
             stream=None, fused_taken=False, signal=None, lr_advance=None, norm_done=False):
        """FusedSGD.step with the trust ratios: one norms launch over the adapted tensors of
        the range, then the update launch (same arguments, same captured behaviour). With the
        gradient guard the sum-of-squares launch comes first (``norm_done`` as in FusedSGD)."""
        if fused_taken:
            raise RuntimeError("LARS: no update is taken in the backward (fused_taken)")
        if lr_advance is None:
            lr_advance = params is None
        if not self._fused:
            out = closure() if closure is not None else None
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
        from ..ops.common import native, stream_handle
        g = self.param_groups[0]
        s = stream.cuda_stream if stream is not None else stream_handle()
        a = self.arena
        rng = tuple(params) if params is not None else (0, len(a.params))
        items, n_items, descs = self._work_table(params)
        tables = self._trust_kw("lars", rng)
        nitems, n_norm = self._norm_table(rng)
        gs = float(self._grad_scale_factor)
        if self.guarded and not norm_done:
            self.grad_sumsq(params, stream)
        if n_norm:
            native().lars_norms(nitems.data_ptr(), n_norm, a.data.data_ptr(), a.grad.data_ptr(),
                                gs, self._trust_partial.data_ptr(), s)
        self._update_launch(items, n_items, s, descs=descs, zero_grad=zero_grad, counter=counter,
                            skip=skip, signal=signal, lr_advance=lr_advance,
                            lars_eta=float(g["trust_coefficient"]), lars_eps=float(g["eps"]),
                            **tables)
        return None

    def load_state_dict(self, sd):
        out = super().load_state_dict(sd)
        if sd.get("param_groups"):
            g, saved = self.param_groups[0], sd["param_groups"][0]
            g["trust_coefficient"] = float(saved.get("trust_coefficient", g["trust_coefficient"]))
            g["eps"] = float(saved.get("eps", g["eps"]))
            g["exclude_1d"] = bool(saved.get("exclude_1d", g["exclude_1d"]))
        return out
