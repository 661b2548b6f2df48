"""Fused multi-tensor SGD.

Reference parity: ``optim.SGD(params, lr=0.1, momentum=0.9, weight_decay=1e-4)``
(part1/main.py:124-125, part3/main.py:176-177): no dampening, no nesterov, momentum buffer
initialised to the first gradient. On the GPU one launch of ``sgd_pack_kernel``
(csrc/kernels/optim.hip) updates the whole flat parameter arena and re-packs every conv weight
into the bf16 MFMA operand layouts the next forward consumes. On the CPU it is exactly
``torch.optim.SGD`` (the oracle).

Learning-rate schedules (``set_schedule``): a captured step bakes the ``lr`` kernel argument in,
so with a schedule attached the fp32 table of optim/schedule.py lives in device memory
(csrc/kernels/api.h LrSched), every update kernel reads this step's entry from it, and the
table's step word advances once per training step: the launch that ends the step stages the
next index and a later launch makes it current (the engine's next batch launch, or a one-thread
launch right behind the update). On the CPU the same fp32 value is written to
``param_groups[0]["lr"]`` before each step.

Gradient guard (``max_grad_norm``, ``skip_nonfinite``; opt-in, all fp32, ``gs`` = ``grad_scale``):

    S    = sum over every parameter element of (g * gs)^2        (arena padding excluded)
    norm = sqrt(S)
    c    = min(1, max_grad_norm / (norm + clip_eps))   if max_grad_norm is set, else 1
    every update uses gs * c where it used gs          (c == 1.0: today's update bit for bit)

and with ``skip_nonfinite`` a step whose norm is not finite (an Inf / NaN gradient, or S beyond
fp32) changes no master, no momentum and no bf16 operand copy; it still clears the gradients
(``zero_grad``), advances the data cursor and the schedule, gives the completion signal, and is
counted (``skipped_steps()``). Without ``skip_nonfinite`` a non-finite norm gives c = 0 or NaN
as the arithmetic says. The captured step has no place between ``backward()`` and ``step()``
where ``clip_grad_norm_`` could stand, so on the GPU the guard lives in the update launch
(csrc/kernels/optim.hip): ``chunk_sums_kernel<false>`` stores one partial sum per 8192-element
chunk, and the guarded instantiation of ``sgd_pack_kernel`` sums all of them in a fixed order in
every block's prologue — no float atomics, no host sync, nothing baked in at capture. An optimizer
with the guard needs the whole gradient before any element moves: no SGD in the backward, no
sharded update (after a reduce-scatter a rank holds a shard of the gradient only, and the
global norm would need one more collective); ``update="allreduce"`` is the plan to use. On the
CPU the norm is taken in fp64 and rounded once to fp32 (the oracle of the kernels), the
gradients are multiplied by gs * c in place and torch.optim.SGD does the rest (the unguarded
CPU path is torch.optim.SGD as is and, as before, does not apply ``grad_scale``).

Weight EMA (``set_ema(decay)``; opt-in): an exponential moving average of the masters in an
fp32 arena of its own with the masters' element index, advanced once per optimizer step,

    e = fma(1 - decay, p_new - e, e)      (fp32; 1 - decay rounded once on the host from fp64)

the lerp form, which leaves e as it is, to the bit, where p_new == e. The masters change inside
a replayed graph, so on the GPU the average is taken in the update launch itself (api.h EmaArgs,
the EMA instantiations of ``sgd_pack_kernel``): the new p is in registers, the cost is one read
and one write of the EMA arena and no dispatch. A step that updates nothing (the ``skip`` word,
a step the guard skipped) leaves it alone. Every update has to run in that launch then
(``updates_in_launch_only``): no SGD in the backward — its WGRAD finishes would need a fourth
pointer in every conv kernel's arguments — and no sharded update. ``swap_ema`` exchanges
masters and average in place (addresses stay: captured graphs stay valid) for evaluation and
checkpoints. On the CPU the same formula runs after each step that was not skipped.

No weight decay on chosen tensors (``no_decay``; opt-in): ``"1d"`` masks every parameter with
``p.dim() <= 1`` (biases, BatchNorm gamma / beta: the two param groups ``{weights, wd}``,
``{1-D tensors, 0}`` of the large-batch recipes), an iterable of parameters masks exactly those.
A masked tensor takes the same rule with ``wd = 0`` — ``d = fma(0, p, g gs)`` here, which equals
torch.optim.SGD's skipped add but for a ``-0`` gradient, which becomes ``+0`` — and nothing else
about its update changes. It is a mask, not a per-tensor decay value or learning rate. A
captured launch bakes the one ``wd`` argument in, so the decision is taken per work item: bit 8
(``NO_DECAY``) of an updating item's kind word (csrc/kernels/optim.hip), OR-ed in by
``_work_table`` (and by ``_elem_table`` / the sharded update's items, cut where the mask
changes), selects ``wd = 0`` for that block. No kernel argument, no launch and no table row is
added, and with the mask off every table is byte for byte what it was. ``set_no_decay`` before
a capture and before a sharded update object is built; the mask travels in
``param_groups[0]["no_decay"]`` (sorted parameter indices) only when it was set.
"""
import contextlib
import itertools

import numpy as np
import torch

from .arena import arena_for
from .schedule import LRSchedule

_GUARD_SHARDED = ("gradient clipping / non-finite step skipping needs the norm of the whole "
                  "gradient: after a reduce-scatter a rank holds only a shard of it, and a global "
                  "norm would need one more collective; use the replicated update, "
                  "update=\"allreduce\"")
_EMA_LAUNCH_ONLY = ("the weight EMA is advanced by the step's own update launch, from the new "
                    "master in its registers")
_SHARDED_LAUNCH_ONLY = ("the sharded updates (ZeRO-1, the bf16-gather update) and element-range "
                        "updates do not carry it; use the replicated update, update=\"allreduce\"")
_BWD_LAUNCH_ONLY = ("an update taken in the backward's WGRAD finishes would not carry it "
                    "(TrainStep keeps opt_in_bwd False)")


def launch_only_sharded(optimizer):
    """The refusal of a sharded or element-range update for an optimizer whose updates run in
    the step's launch only, naming the reason (the weight EMA, AdamW)."""
    return optimizer.launch_only_reason + ": " + _SHARDED_LAUNCH_ONLY


def one_minus_decay(decay):
    """float32(1 - decay): the subtraction in fp64, rounded once (the kernel's argument)."""
    return float(np.float32(1.0 - float(decay)))


def fma32(a, b, c):
    """fp32 fma(a, b, c) of fp32 tensors (``a`` may be a Python float holding an fp32 value),
    correctly rounded: the product is exact in fp64, the fp64 sum is rounded to odd (its TwoSum
    error says whether it was inexact), and a round-to-odd value with 29 spare bits rounds to
    fp32 as the exact sum would."""
    a64 = a.double() if torch.is_tensor(a) else float(a)
    prod, c64 = b.double() * a64, c.double()
    s = c64 + prod
    bb = s - c64
    err = (c64 - (s - bb)) + (prod - bb)
    even = (s.view(torch.int64) & 1) == 0
    inf = torch.full_like(s, float("inf"))
    odd = torch.nextafter(s, torch.where(err > 0, inf, -inf))
    return torch.where((err != 0) & even, odd, s).float()


def ema_lerp(e, p, omd):
    """The EMA's step on fp32 tensors, as the update kernel takes it: fma(omd, p - e, e) with
    ``omd`` = ``one_minus_decay(decay)``; two roundings, the subtraction and the fma."""
    return fma32(omd, p - e, e)


class FusedSGD(torch.optim.SGD):
    # True for an optimizer whose update of one element needs the whole tensor (optim/lars.py):
    # the updates that split tensors across ranks or run before a gradient is complete refuse it
    needs_whole_tensors = False

    def __init__(self, params, lr=0.1, momentum=0.0, dampening=0.0, weight_decay=0.0,
                 nesterov=False, grad_scale=1.0, max_grad_norm=None, clip_eps=1e-6,
                 skip_nonfinite=False, no_decay=None):
        params = list(params)
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening,
                         weight_decay=weight_decay, nesterov=nesterov)
        self._no_decay = frozenset()  # masked parameter indices (arena order)
        self._grad_scale_factor = grad_scale
        self._fused = bool(params) and params[0].is_cuda
        if self._fused:
            if dampening != 0.0:
                raise ValueError("fused SGD supports dampening=0 only")
            if len(self.param_groups) != 1:
                raise ValueError("fused SGD supports a single param group")
            self.arena = arena_for(params)
            self.momentum_buffer = torch.zeros_like(self.arena.data)
            # first chunk of each parameter, numbered over the arena: the slots of the guard's
            # and LARS' per-chunk partial sums
            first = list(itertools.accumulate((-(-n // self.CHUNK) for n in self.arena.numels),
                                              initial=0))
            self._chunk0, self._n_chunks = first[:-1], first[-1]
        else:
            # CPU: plain torch.optim.SGD; the flat arena (if the DDP wrapper built one) serves the
            # element-range update of the ZeRO-1 path (step_elements)
            self.arena = getattr(params[0], "_ddp_amd_arena", None) if params else None
        self._schedule = None
        self._lr_step = 0    # host mirror of the device step word: steps taken so far
        self._lr_dev = None  # device LrSched: int32 [step, n, next, pad] + n fp32 rates
        self._guard_dev = None
        self._elem_tables = {}
        self._guard_cpu = [float("nan"), 1.0, 0]  # norm, coefficient, skipped steps
        self._set_guard(max_grad_norm, clip_eps, skip_nonfinite)
        self._ema = None        # the EMA arena (set_ema allocates it once)
        self._ema_decay = None  # None: off
        if no_decay is not None:
            self.set_no_decay(no_decay)

    @property
    def grad_scale_factor(self):
        """The constructor's ``grad_scale``: the factor every update site multiplies the
        gradient by before using it (a launch argument: set it before capturing). Gradient
        accumulation over K micro-batches sets float32(grad_scale / K) for the step that
        consumes the sum (engine/step.py). Not named ``grad_scale``: torch.optim.Optimizer
        reads an attribute of that name as the AMP gradient scaler's tensor."""
        return self._grad_scale_factor

    @grad_scale_factor.setter
    def grad_scale_factor(self, v):
        self._grad_scale_factor = float(v)

    # ------------------------------------------------------------------------- no-decay mask
    NO_DECAY = 0x100  # bit 8 of an updating work item's kind word (optim.hip kItemNoDecay)

    def set_no_decay(self, spec):
        """Choose the tensors that are not weight-decayed: ``None`` (none), ``"1d"`` (every
        parameter with ``p.dim() <= 1``), an iterable of this optimizer's parameters (matched by
        identity), or — what a state dict carries — a list of parameter indices. The mask is
        baked into the work-item tables: call it before a capture and before a sharded update
        object is built; every cached work, side, norm and element table is dropped.
        ``param_groups[0]["no_decay"]`` (sorted indices) exists only while a mask is set."""
        if len(self.param_groups) != 1:
            raise ValueError("the no-decay mask supports a single param group")
        g = self.param_groups[0]
        params = g["params"]
        if spec is None:
            idx = None
        elif isinstance(spec, str):
            if spec != "1d":
                raise ValueError(f"no_decay = {spec!r}: None, \"1d\" or an iterable of parameters")
            idx = [i for i, p in enumerate(params) if p.dim() <= 1]
        else:
            where = {id(p): i for i, p in enumerate(params)}
            idx = []
            for t in spec:
                if torch.is_tensor(t):
                    if id(t) not in where:
                        raise ValueError("no_decay: a tensor that is not a parameter of this "
                                         "optimizer")
                    idx.append(where[id(t)])
                elif isinstance(t, int) and not isinstance(t, bool) and 0 <= t < len(params):
                    idx.append(t)
                else:
                    raise ValueError(f"no_decay: {t!r} is neither a parameter of this optimizer "
                                     "nor a parameter index")
        self._no_decay = frozenset(idx or ())
        if idx is None:
            g.pop("no_decay", None)
            self.defaults.pop("no_decay", None)
        else:
            g["no_decay"] = sorted(self._no_decay)
            self.defaults["no_decay"] = []  # (a group added later masks nothing)
        # every table that carries the flag
        self._table_key = None
        self._elem_tables = {}
        for name in ("_sumsq_tables", "_norm_tables"):
            if hasattr(self, name):
                setattr(self, name, {})

    @property
    def no_decay_mask(self):
        """One bool per parameter in arena order: True where the tensor is not decayed."""
        return [i in self._no_decay for i in range(len(self.param_groups[0]["params"]))]

    @property
    def no_decay_name(self):
        """The mask as --metrics records name it: None (off), "1d" (exactly the parameters with
        ``p.dim() <= 1``), else "custom"."""
        if not self._no_decay:
            return None
        one_d = {i for i, p in enumerate(self.param_groups[0]["params"]) if p.dim() <= 1}
        return "1d" if self._no_decay == one_d else "custom"

    def _wd_of(self, i):
        """Parameter i's weight decay: the group's, or 0.0 under the mask."""
        return 0.0 if i in self._no_decay else float(self.param_groups[0]["weight_decay"])

    def _decay_runs(self, lo, hi):
        """Arena elements [lo, hi) cut where the mask changes: (start, end, masked) runs. A
        tensor's alignment padding goes with the tensor before it (parallel/zero.py _tensors)."""
        a = self.arena
        if not self._no_decay:
            return [(lo, hi, False)]
        ends = list(a.offsets[1:]) + [a.total]
        runs = []
        for i, (t0, t1) in enumerate(zip(a.offsets, ends)):
            s, e, nd = max(lo, t0), min(hi, t1), i in self._no_decay
            if s >= e:
                continue
            if runs and runs[-1][2] == nd and runs[-1][1] == s:
                runs[-1] = (runs[-1][0], e, nd)
            else:
                runs.append((s, e, nd))
        return runs

    # ------------------------------------------------------------------------ gradient guard
    CHUNK = 8192  # elements per elementwise item and per chunk-sum block (optim.hip kNormChunk)

    def _set_guard(self, max_grad_norm, clip_eps, skip_nonfinite):
        """Set the guard's options (constructor, load_state_dict). They live in
        ``param_groups[0]`` only when one of them is on: a plain optimizer's state_dict is what
        it was. GPU: the partial and statistics buffers are allocated ONCE, so their addresses
        survive re-captures; the options are launch arguments (capture after changing them)."""
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be positive")
        if float(clip_eps) < 0.0:
            raise ValueError("clip_eps must be >= 0")
        on = max_grad_norm is not None or bool(skip_nonfinite)
        g = self.param_groups[0] if self.param_groups else {}
        if on:
            hyper = {"max_grad_norm": None if max_grad_norm is None else float(max_grad_norm),
                     "clip_eps": float(clip_eps), "skip_nonfinite": bool(skip_nonfinite)}
            self.defaults.update(hyper)
            g.update(hyper)
            # the norm of the WHOLE gradient comes before any element's update
            self.needs_whole_tensors = True
        else:
            for k in ("max_grad_norm", "clip_eps", "skip_nonfinite"):
                g.pop(k, None)
                self.defaults.pop(k, None)
            self.__dict__.pop("needs_whole_tensors", None)
        if on and self._fused and self._guard_dev is None:
            dev = self.arena.data.device
            self._sumsq_partial = torch.zeros(max(self._n_chunks, 1), dtype=torch.float32,
                                              device=dev)
            self._guard_dev = torch.zeros(4, dtype=torch.float32, device=dev)
            self._guard_dev[1] = 1.0
            self._sumsq_tables = {}

    @property
    def guarded(self):
        """Either guard option is on (the update launch is the clipped instantiation)."""
        g = self.param_groups[0]
        return g.get("max_grad_norm") is not None or bool(g.get("skip_nonfinite", False))

    def grad_norm(self):
        """2-norm of the last step's scaled gradient, before clipping (GPU: a view of the
        device statistics the update launch writes; no sync)."""
        if self._guard_dev is not None:
            return self._guard_dev[0]
        return torch.tensor(self._guard_cpu[0], dtype=torch.float32)

    def clip_coef(self):
        """Clip coefficient c of the last step (1.0: not clipped)."""
        if self._guard_dev is not None:
            return self._guard_dev[1]
        return torch.tensor(self._guard_cpu[1], dtype=torch.float32)

    def skipped_steps(self):
        """Steps skipped for a non-finite gradient norm so far."""
        if self._guard_dev is not None:
            return self._guard_dev.view(torch.int32)[2]
        return torch.tensor(self._guard_cpu[2], dtype=torch.int32)

    def _chunk_table(self, rng, keep=None):
        """Work items of a chunk-sum launch (the guard's sum of squares, LARS' norms) over
        parameters [i0, i1), those with ``keep[i]`` if given: one per chunk, {arena offset,
        count, global chunk number, 1 under the no-decay mask else 0}. The fourth field is read
        by LAMB's norms launch only. Returns (device table or None, rows)."""
        a = self.arena
        rows = [[a.offsets[i] + s0, min(self.CHUNK, a.numels[i] - s0), self._chunk0[i] + c,
                 int(i in self._no_decay)]
                for i in range(*rng) if keep is None or keep[i]
                for c, s0 in enumerate(range(0, a.numels[i], self.CHUNK))]
        return (torch.tensor(rows, dtype=torch.int32, device=a.data.device) if rows else None,
                len(rows))

    def _sumsq_table(self, rng):
        """``_chunk_table`` over every parameter of the range; cached per range."""
        if rng not in self._sumsq_tables:
            self._sumsq_tables[rng] = self._chunk_table(rng)
        return self._sumsq_tables[rng]

    def grad_sumsq(self, params=None, stream=None):
        """Launch the sum-of-squares pass over parameters ``params = (i0, i1)`` (default: all)
        on ``stream``: what ``step`` does first unless ``norm_done=True`` (the pipelined DDP step
        runs it per bucket behind the bucket's all-reduce)."""
        from ..ops.common import native, stream_handle
        a = self.arena
        rng = tuple(params) if params is not None else (0, len(a.params))
        items, n = self._sumsq_table(rng)
        if n:
            native().grad_sumsq(items.data_ptr(), n, a.grad.data_ptr(),
                                float(self._grad_scale_factor), self._sumsq_partial.data_ptr(),
                                stream.cuda_stream if stream is not None else stream_handle())

    def _clip_kw(self, count):
        """Extra arguments of a native update launch: none without the guard (the launch is
        then exactly the unguarded one). ``count``: the launch ends the step."""
        if not self.guarded:
            return {}
        g = self.param_groups[0]
        mx = g.get("max_grad_norm")
        flags = (1 if mx is not None else 0) | (2 if g.get("skip_nonfinite") else 0) | \
            (4 if count else 0)
        return {"clip_partial": self._sumsq_partial.data_ptr(), "clip_chunks": self._n_chunks,
                "clip_max_norm": float(mx) if mx is not None else 0.0,
                "clip_eps": float(g.get("clip_eps", 1e-6)), "clip_flags": flags,
                "clip_stats": self._guard_dev.data_ptr()}

    @torch.no_grad()
    def _cpu_guard(self, lr_advance):
        """CPU: the guard's formula on the gradients of every parameter. Returns (c, skipped);
        a skipped step is counted here."""
        g = self.param_groups[0]
        gs = float(self._grad_scale_factor)
        grads = [p.grad for p in g["params"] if p.grad is not None]
        # fp64 sum, rounded ONCE to fp32: the oracle of the kernels' fp32 sums
        S = sum(((gr.double() * gs) ** 2).sum() for gr in grads) if grads else torch.zeros(())
        S = torch.as_tensor(S, dtype=torch.float64).to(torch.float32)  # beyond fp32: inf
        norm = S.sqrt()
        c = torch.ones((), dtype=torch.float32)
        if g.get("max_grad_norm") is not None:
            q = torch.tensor(g["max_grad_norm"], dtype=torch.float32) / \
                (norm + torch.tensor(g["clip_eps"], dtype=torch.float32))
            c = torch.clamp(q, max=1.0)  # NaN stays NaN
        skipped = bool(g.get("skip_nonfinite")) and not bool(torch.isfinite(norm))
        self._guard_cpu[0], self._guard_cpu[1] = float(norm), float(c)
        if skipped and lr_advance:
            self._guard_cpu[2] += 1
        return c, skipped

    def _cpu_scale_grads(self, c):
        """grad *= gs * c in place (what ``clip_grad_norm_`` does with c), unless it is 1."""
        f = torch.tensor(float(self._grad_scale_factor), dtype=torch.float32) * c
        if float(f) != 1.0:
            for p in self.param_groups[0]["params"]:
                if p.grad is not None:
                    p.grad.mul_(f)

    # ------------------------------------------------------------------------------ weight EMA
    def _ema_layout(self):
        """(offsets, total) of the EMA arena: the parameter arena's where there is one (GPU, or
        the DDP wrapper's on the CPU), else the parameters back to back."""
        if self.arena is not None:
            return self.arena.offsets, self.arena.total
        numels = [p.numel() for p in self.param_groups[0]["params"]]
        off = list(itertools.accumulate(numels, initial=0))
        return off[:-1], off[-1]

    def _ema_view(self, i):
        """Tensor i of the EMA arena in the parameter's logical shape."""
        if self.arena is not None:
            return self.arena.shaped(self._ema, i)
        p = self.param_groups[0]["params"][i]
        o = self._ema_layout()[0][i]
        return self._ema[o:o + p.numel()].view(p.shape)

    def set_ema(self, decay):
        """Switch the weight EMA on with ``0 < decay < 1`` (``None``: off). The EMA arena is
        allocated ONCE, so its address survives re-captures, and seeded with a copy of the
        current masters: call it once the weights are final (after the DDP wrapper's rank-0
        broadcast, after a checkpoint load). ``ema_decay`` lives in ``param_groups[0]`` only
        when the EMA is on: a plain optimizer's state_dict is what it was. The decay is a
        launch argument (capture after changing it)."""
        g = self.param_groups[0]
        if decay is None:
            self._ema_decay = None
            g.pop("ema_decay", None)
            self.defaults.pop("ema_decay", None)
            return
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise ValueError("ema decay must be in (0, 1)")
        if len(self.param_groups) != 1:
            raise ValueError("the weight EMA supports a single param group")
        params = g["params"]
        if self._ema is None:
            total = self._ema_layout()[1]
            self._ema = torch.zeros(total, dtype=torch.float32, device=params[0].device)
        with torch.no_grad():
            if self.arena is not None:
                self._ema.copy_(self.arena.data)
            else:
                for i, p in enumerate(params):
                    self._ema_view(i).copy_(p.detach())
        self._ema_decay = decay
        g["ema_decay"] = decay
        self.defaults["ema_decay"] = decay

    @property
    def ema_decay(self):
        """The EMA's decay, or None when it is off."""
        return self._ema_decay

    @property
    def ema(self):
        """The EMA arena: flat fp32, the masters' element index (None before ``set_ema``)."""
        return self._ema

    # why every update of this optimizer class has to run in the step's own update launch,
    # whatever its options (optim/adamw.py: the rule exists there only); None: no such reason
    _rule_launch_only = None

    @property
    def launch_only_reason(self):
        """Why every update has to run in the step's own update launch (the optimizer's rule,
        the weight EMA, or both), or None."""
        why = [w for w in (self._rule_launch_only,
                           _EMA_LAUNCH_ONLY if self._ema_decay is not None else None) if w]
        return "; ".join(why) if why else None

    @property
    def updates_in_launch_only(self):
        """Every update of this optimizer has to run in the step's own update launch (the
        weight EMA is taken there, AdamW's rule exists there only): no SGD in the backward, no
        sharded or element-range update. ``launch_only_reason`` says why."""
        return self.launch_only_reason is not None

    def _ema_kw(self):
        """Extra arguments of a native update launch: none with the EMA off (the launch is then
        exactly the plain one)."""
        if self._ema_decay is None:
            return {}
        return {"ema": self._ema.data_ptr(),
                "ema_one_minus_decay": one_minus_decay(self._ema_decay)}

    @torch.no_grad()
    def _cpu_ema(self, rng=None):
        """CPU: advance the EMA of parameters ``rng`` (default: all) after a step that was taken."""
        if self._ema_decay is None:
            return
        omd = one_minus_decay(self._ema_decay)
        params = self.param_groups[0]["params"]
        for i in range(*(rng if rng is not None else (0, len(params)))):
            if params[i].grad is None:
                continue
            e = self._ema_view(i)
            e.copy_(ema_lerp(e.contiguous(), params[i].detach().float().contiguous(), omd))

    def _need_ema(self):
        if self._ema_decay is None:
            raise RuntimeError("the weight EMA is off (set_ema)")

    def ema_state(self, model=None):
        """The EMA per parameter, fp32 on the host in the parameter's logical shape: under the
        ``model``'s state_dict keys, or under the optimizer state_dict's parameter indices."""
        self._need_ema()
        params = self.param_groups[0]["params"]
        keys = self._ema_keys(model)
        return {keys[i]: self._ema_view(i).detach().cpu().contiguous().clone()
                for i in range(len(params))}

    def _ema_keys(self, model):
        params = self.param_groups[0]["params"]
        if model is None:
            return list(range(len(params)))
        name = {id(p): k for k, p in model.named_parameters()}
        missing = [i for i, p in enumerate(params) if id(p) not in name]
        if missing:
            raise KeyError(f"parameters {missing} of the optimizer are not the model's")
        return [name[id(p)] for p in params]

    @torch.no_grad()
    def load_ema_state(self, state, model=None):
        """Inverse of ``ema_state``: every parameter's entry is required."""
        self._need_ema()
        for i, k in enumerate(self._ema_keys(model)):
            v = state[k] if k in state else state[str(k)]
            e = self._ema_view(i)
            e.copy_(torch.as_tensor(v).to(torch.float32).reshape(e.shape))

    @torch.no_grad()
    def swap_ema(self):
        """Exchange the masters and the EMA in place and rebuild the bf16 operand copies from
        the new masters. Addresses stay, so captured graphs stay valid; two swaps restore the
        masters and every operand copy bit for bit. Plumbing outside the hot path."""
        self._need_ema()
        if self.arena is not None:
            tmp = self.arena.data.clone()
            self.arena.data.copy_(self._ema)
            self._ema.copy_(tmp)
            if self._fused:
                self.repack()
            return
        for i, p in enumerate(self.param_groups[0]["params"]):
            e = self._ema_view(i)
            tmp = p.detach().clone()
            p.copy_(e)
            e.copy_(tmp)

    @contextlib.contextmanager
    def ema_weights(self):
        """The model runs on the averaged weights inside (``swap_ema`` around the block)."""
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    # ------------------------------------------------------------------ learning-rate schedule
    def set_schedule(self, schedule, step=0):
        """Attach an ``LRSchedule`` (``None`` detaches): from now on step k of the run uses
        ``schedule.table()[min(k, total_steps - 1)]``, starting at k = ``step``. GPU: uploads the
        table into the optimizer's device structure — allocated ONCE and reused, so its address
        survives re-captures (a longer table than any before re-allocates it: capture after
        attaching) — and sets its step word; the host keeps a mirror of the step index, counted
        per ``step()`` / replay, so ``current_lr()`` needs no device sync."""
        self._schedule = schedule
        self._lr_step = int(step)
        if schedule is None:
            return
        table = schedule.table()
        if self._fused:
            n = table.numel()
            if self._lr_dev is None or self._lr_dev.numel() < 4 + n:
                self._lr_dev = torch.zeros(4 + n, dtype=torch.int32, device=self.arena.data.device)
            self._lr_dev[4:4 + n].view(torch.float32).copy_(table)
            self._lr_dev[:4].copy_(torch.tensor([int(step), n, int(step), 0], dtype=torch.int32))

    @property
    def schedule(self):
        return self._schedule

    @property
    def lr_step(self):
        """Steps counted so far (host mirror; the index of the NEXT step's learning rate)."""
        return self._lr_step

    def set_lr_step(self, k):
        """Move the schedule to step k: the device step word and its host mirror (state
        rollbacks after warm-up / capture / validation steps, checkpoint restore)."""
        self._lr_step = int(k)
        if self._schedule is not None and self._fused:
            self._lr_dev[0:3:2].fill_(int(k))  # step and next

    def lr_step_device(self):
        """Steps taken according to the device (LrSched::next; one device read: tests and
        consistency checks)."""
        return int(self._lr_dev[2].item()) if self._sched_ptr() else self._lr_step

    def current_lr(self):
        """Learning rate the next step uses (no device sync)."""
        if self._schedule is None:
            return float(self.param_groups[0]["lr"])
        return self._schedule.lr_at(self._lr_step)

    def count_step(self):
        """Advance the host mirror by one training step. Called by every eager step and by the
        owner of a captured graph after each replay; a launch that is only being captured runs
        nothing on the device and is not counted."""
        if self._schedule is None:
            return
        if self._fused and torch.cuda.is_current_stream_capturing():
            return
        self._lr_step += 1

    # ------------------------------------------------------------- state snapshot and rollback
    def _state_arenas(self):
        """The optimizer's own arenas on the GPU, in snapshot order: momentum (optim/adamw.py
        adds the second moment)."""
        return [self.momentum_buffer]

    def state_snapshot(self):
        """Clones of everything a training step changes in the optimizer (GPU): momentum (and
        AdamW's second moment), the schedule's step, the weight EMA if it is on. For the
        roll-backs around warm-up, capture, validation and profiling steps."""
        return {"arenas": [t.clone() for t in self._state_arenas()], "lr_step": self._lr_step,
                "ema": self._ema.clone() if self._ema_decay is not None else None}

    @torch.no_grad()
    def restore_state(self, snap):
        """Inverse of ``state_snapshot``, in place: addresses stay, captured graphs stay valid."""
        for t, v in zip(self._state_arenas(), snap["arenas"]):
            t.copy_(v)
        self.set_lr_step(snap["lr_step"])
        if snap["ema"] is not None:
            self._ema.copy_(snap["ema"])

    def _sched_ptr(self):
        return self._lr_dev.data_ptr() if (self._schedule is not None and self._fused) else 0

    def _sched_kw(self, advance):
        """Extra arguments of a native update launch: none without a schedule (the launch is
        then exactly the unscheduled one)."""
        ptr = self._sched_ptr()
        return {"sched": ptr, "sched_advance": int(bool(advance))} if ptr else {}

    def commit_lr_step(self, stream=None):
        """Make a staged step current now (one-thread launch): for an eager step that follows
        ``lr_advance="stage"`` steps without the loader's batch launch in between."""
        if self._sched_ptr():
            from ..ops.common import native, stream_handle
            native().counter_add(0, 0, stream if stream is not None else stream_handle(),
                                 sched=self._sched_ptr(), sched_mode=2)

    def _sched_commit(self, advance, stream):
        """After an update launch that staged the next step (``advance``): make it current with
        a one-thread launch, unless the caller leaves that to the next step's batch launch
        (``advance == "stage"``: data/loader.py fill(lr_sched=...), engine/step.py)."""
        if advance and advance != "stage" and self._sched_ptr():
            from ..ops.common import native
            native().counter_add(0, 0, stream, sched=self._sched_ptr(), sched_mode=2)
        if advance:
            self.count_step()

    def _cpu_lr(self):
        """CPU: this step's fp32 table entry into the param group (what torch.optim.SGD reads)."""
        if self._schedule is not None:
            self.param_groups[0]["lr"] = self._schedule.lr_at(self._lr_step)
        return float(self.param_groups[0]["lr"])

    def _packs(self):
        return [p._ddp_amd_pack() for p in self.arena.params if hasattr(p, "_ddp_amd_pack")]

    def repack(self):
        """Rebuild every bf16 conv-weight copy from the fp32 master weights (after the master
        weights were written outside the optimizer, e.g. a state rollback or checkpoint load)."""
        descs = self._packs()
        if descs and self.arena.data.is_cuda:
            from ..ops.common import native, stream_handle
            native().pack_conv_weights(descs, stream_handle())

    def register_in_backward(self):
        """SGD in the backward (engine/step.py TrainStep, one GPU): hand every conv weight whose
        bf16 copy has the master's index order to the kernel library, which applies its update
        in the WGRAD split-K finish that completes its gradient (conv_igemm.hip SgdFuse). Active
        until unregister_in_backward(); ``step(fused_taken=True)`` then skips the tensors whose
        finish took it (native sgd_fuse_taken). Not with gradient accumulation: a finish takes
        its step from its own sum alone (engine/step.py keeps opt_in_bwd False for K > 1)."""
        if self.guarded:
            raise RuntimeError("gradient clipping / non-finite step skipping cannot run in the "
                               "backward: the norm exists only once the whole gradient does "
                               "(TrainStep keeps opt_in_bwd False)")
        if self.updates_in_launch_only:
            raise RuntimeError(self.launch_only_reason + ": " + _BWD_LAUNCH_ONLY)
        from ..ops.common import native
        a, g = self.arena, self.param_groups[0]
        nat = native()
        nat.sgd_fuse_register(0, clear=1)
        self._bwd_index = {}
        base_g, base_p = a.grad.data_ptr(), a.data.data_ptr()
        base_b = self.momentum_buffer.data_ptr()
        sched = {"sched": self._sched_ptr()} if self._sched_ptr() else {}
        for i, p in enumerate(a.params):
            if not hasattr(p, "_ddp_amd_pack"):
                continue
            pp, wc, wt, K, Cr, C, R, S, krsc = p._ddp_amd_pack()
            if wt or not wc or not (krsc or R * S == 1) or pp != base_p + 4 * a.offsets[i]:
                continue
            dw = base_g + 4 * a.offsets[i]
            nat.sgd_fuse_register(dw, pp, base_b + 4 * a.offsets[i], wc, float(g["lr"]),
                                  float(g["momentum"]), self._wd_of(i),
                                  float(self._grad_scale_factor), int(bool(g["nesterov"])),
                                  **sched)
            self._bwd_index[dw] = i
        nat.sgd_fuse_begin()

    def unregister_in_backward(self):
        from ..ops.common import native
        native().sgd_fuse_register(0, clear=1)

    def _fused_in_backward(self):
        """Parameter indices whose update a WGRAD finish applied since register_in_backward."""
        from ..ops.common import native
        idx = getattr(self, "_bwd_index", {})
        return frozenset(idx[d] for d in native().sgd_fuse_taken() if d in idx)

    def _master_in_backward(self):
        """Parameter indices whose fp32 master (and momentum) a backward pair's unsplit WGRAD
        epilogue updated: the step's launch re-packs only their bf16 operand copy."""
        from ..ops.common import native
        idx = getattr(self, "_bwd_index", {})
        return frozenset(idx[d] for d in native().sgd_fuse_taken_master() if d in idx)

    def _work_table(self, prange=None, exclude=frozenset(), pack_only=frozenset()):
        """Device work-item table of the fused SGD + re-pack kernel (rebuilt when the set of
        packed conv weights changes, e.g. after the model's fused plan is first built).
        ``prange = (i0, i1)`` restricts it to parameters i0 <= i < i1 (one DDP bucket: the
        pipelined step updates each bucket as soon as its all-reduce is done); ``exclude`` =
        parameter indices updated elsewhere (SGD in the backward); ``pack_only`` (a subset of
        ``exclude``) = those whose bf16 operand copy is still to be re-packed here (item 5)."""
        from ..ops.common import native
        a = self.arena
        key = (tuple(self._packs()), self._no_decay) if self._no_decay else tuple(self._packs())
        if getattr(self, "_table_key", None) != key:
            self._tables = {}
            self._table_key = key
            descs, per_param = [], [[] for _ in a.params]
            for i, p in enumerate(a.params):
                if not hasattr(p, "_ddp_amd_pack"):
                    continue
                pp, wc, wt, K, Cr, C, R, S, krsc = p._ddp_amd_pack()
                if pp != a.data.data_ptr() + 4 * a.offsets[i] or (R * S > 1 and bool(krsc) != a.krsc[i]):
                    raise RuntimeError("packed conv weight is not a view into the parameter arena")
                d = len(descs)
                descs.append([a.offsets[i], K, Cr, C, R, S, wc, wt, int(krsc), 0, 0, 0])
                n = a.numels[i]
                if not wt and C == Cr and (krsc or R * S == 1) and n % 4 == 0:
                    # bf16 copy in the master's own index order: elementwise items
                    for s0 in range(0, n, self.CHUNK):
                        per_param[i].append([2, s0, min(self.CHUNK, n - s0), d])
                    continue
                TK, TC = native().sgd_tile_dims(R * S)
                if TK * TC * R * S > native().sgd_tile_limit():
                    self._table_key = None  # (nothing was built: the next call refuses again)
                    raise ValueError(
                        f"parameter {i} (conv weight {K}x{Cr}x{R}x{S}, operand channels {C}): a "
                        f"{TK} x {TC} tile of a {R}x{S} filter needs {TK * TC * R * S} floats, "
                        f"the re-pack kernel's tile holds {native().sgd_tile_limit()}")
                for k0 in range(0, K, TK):
                    for c0 in range(0, C, TC):
                        per_param[i].append([1, d, k0, c0])
            for i in range(len(a.params)):
                if per_param[i]:
                    continue
                o, n = a.offsets[i], a.numels[i]
                for s in range(0, n, self.CHUNK):
                    per_param[i].append([0, o + s, min(self.CHUNK, n - s), 0])
            for i in self._no_decay:  # the block of a masked tensor's item runs with wd = 0
                for it in per_param[i]:
                    it[0] |= self.NO_DECAY
            self._per_param = per_param
            dev = a.data.device
            self._descs = torch.tensor(descs if descs else [[0] * 12], dtype=torch.int64, device=dev)
        rng = tuple(prange) if prange is not None else (0, len(a.params))
        t = self._tables.get((rng, exclude, pack_only))
        if t is None:
            keep = [i for i in range(*rng) if i not in exclude]
            packs = [i for i in range(*rng) if i in pack_only]
            for i in packs:
                if not self._per_param[i] or any(it[0] & 0xff != 2 for it in self._per_param[i]):
                    raise RuntimeError(f"parameter {i}: no elementwise re-pack layout")
            # conv re-pack items first (the heavier tiles start early), then elementwise items
            # (owner parameter, item) pairs; a re-pack-only item updates nothing: owner -1
            own = [(i, it) for i in keep for it in self._per_param[i] if it[0] & 0xff != 0] + \
                  [(-1, [5] + it[1:]) for i in packs for it in self._per_param[i]] + \
                  [(i, it) for i in keep for it in self._per_param[i] if it[0] & 0xff == 0]
            sel = [it for _, it in own]
            if not sel and not exclude:
                raise ValueError(f"no parameters in range {rng}")
            items = (torch.tensor(sel, dtype=torch.int32, device=a.data.device) if sel
                     else None)
            t = (items, len(sel), [i for i, _ in own])
            self._tables[(rng, exclude, pack_only)] = t
        return t[0], t[1], self._descs

    def _elem_table(self, lo, hi):
        """Plain fp32 SGD items over arena elements [lo, hi) (no bf16 re-pack): the ZeRO-1
        shard update (parallel/zero.py). Under the no-decay mask the chunks are cut where the
        mask changes and the masked runs carry the flag."""
        t = self._elem_tables.get((lo, hi))
        if t is None:
            items = [[self.NO_DECAY if nd else 0, s0, min(self.CHUNK, e - s0), 0]
                     for s, e, nd in self._decay_runs(lo, hi) for s0 in range(s, e, self.CHUNK)]
            if not items:
                raise ValueError("empty element range")
            t = (torch.tensor(items, dtype=torch.int32, device=self.arena.data.device), len(items))
            self._elem_tables[(lo, hi)] = t
        return t

    @torch.no_grad()
    def step_elements(self, lo, hi, stream=None, zero_grad=False, counter=None, skip=None,
                      lr_advance=True):
        """SGD (fp32 master + momentum only) on arena elements [lo, hi): one launch on the GPU,
        torch.optim.SGD's exact per-element math on the flat slices on the CPU.
        ``lr_advance=False``: not the training step's last update (an attached schedule stays
        at this step for the launches that follow); ``"stage"``: as in ``step``."""
        if self.guarded:
            raise ValueError(_GUARD_SHARDED)
        if self.updates_in_launch_only:
            raise ValueError(launch_only_sharded(self))
        g = self.param_groups[0]
        lr, m, wd = float(g["lr"]), float(g["momentum"]), float(g["weight_decay"])
        a = self.arena
        if not self._fused:
            lr = self._cpu_lr()
            if lr_advance:
                self.count_step()
            p, gr = a.data[lo:hi], a.grad[lo:hi]
            d = gr
            if wd != 0:
                d = gr.clone()
                for s, e, nd in self._decay_runs(lo, hi):
                    if not nd:
                        d[s - lo:e - lo].add_(a.data[s:e], alpha=wd)
            if m != 0:
                if not hasattr(self, "_flat_buf"):
                    self._flat_buf = torch.zeros_like(a.data)
                    self._flat_init = torch.zeros(a.total, dtype=torch.bool)
                buf = self._flat_buf[lo:hi]
                if bool(self._flat_init[lo:hi].all()):
                    buf.mul_(m).add_(d)
                else:
                    buf.copy_(d)
                    self._flat_init[lo:hi] = True
                d = buf
            p.add_(d, alpha=-lr)
            if zero_grad:
                gr.zero_()
            return
        from ..ops.common import stream_handle
        s = stream.cuda_stream if stream is not None else stream_handle()
        items, n_items = self._elem_table(lo, hi)
        self._update_launch(items, n_items, s, zero_grad=zero_grad, counter=counter, skip=skip,
                            lr_advance=lr_advance)

    def _cpu_masked_step(self, closure):
        """CPU under the no-decay mask: torch.optim.SGD.step with the group taken as its two
        sub-lists, the decayed parameters with ``weight_decay`` and the masked ones with 0 —
        torch's own functional ``sgd`` both times, the momentum buffers in ``self.state`` in
        torch's layout: bit for bit torch.optim.SGD with the two param groups."""
        from torch.optim.sgd import sgd
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g = self.param_groups[0]
        for masked in (False, True):
            sub = dict(g, params=[p for i, p in enumerate(g["params"])
                                  if (i in self._no_decay) == masked],
                       weight_decay=0.0 if masked else g["weight_decay"])
            params, grads, bufs = [], [], []
            sparse = self._init_group(sub, params, grads, bufs)
            if not params:
                continue
            sgd(params, grads, bufs, weight_decay=sub["weight_decay"], momentum=g["momentum"],
                lr=g["lr"], dampening=g["dampening"], nesterov=g["nesterov"],
                maximize=g["maximize"], has_sparse_grad=sparse, foreach=g["foreach"],
                fused=g["fused"], grad_scale=None, found_inf=None)
            if g["momentum"] != 0:
                for p, b in zip(params, bufs):
                    self.state[p]["momentum_buffer"] = b
        return loss

    def _descs_ptr(self):
        return self._work_table()[2].data_ptr()

    def _update_launch(self, items, n_items, s, descs=None, zero_grad=False, counter=None,
                       skip=None, signal=None, lr_advance=False, **native_kw):
        """The one native update launch: ``n_items`` work items on the raw stream ``s`` with
        this optimizer's hyper-parameters and ``grad_scale_factor``. Step-level options as in
        ``step``; ``descs``: the table a ``_work_table`` call just returned (default: looked
        up); ``native_kw``: further native keywords (LARS', the sharded update's ``shadow`` /
        ``slot``). The schedule's, the guard's and the EMA's keywords go in only when they are
        on."""
        from ..ops.common import native
        g, a = self.param_groups[0], self.arena
        native().sgd_pack(items.data_ptr(), n_items,
                          descs.data_ptr() if descs is not None else self._descs_ptr(),
                          a.data.data_ptr(), a.grad.data_ptr(), self.momentum_buffer.data_ptr(),
                          float(g["lr"]), float(g["momentum"]), float(g["weight_decay"]),
                          float(self._grad_scale_factor), int(bool(g["nesterov"])), s,
                          zero_grad=int(bool(zero_grad)),
                          counter=int(counter[0]) if counter else 0,
                          delta=int(counter[1]) if counter else 0,
                          skip=int(skip) if skip else 0,
                          done=int(signal[0]) if signal else 0,
                          signal=int(signal[1]) if signal else 0, **native_kw,
                          **self._sched_kw(lr_advance), **self._clip_kw(lr_advance),
                          **self._ema_kw())
        self._sched_commit(lr_advance, s)

    def repack_params(self, i0, i1, stream=None):
        """Rebuild the bf16 operand copies of the conv weights among parameters [i0, i1)."""
        descs = [p._ddp_amd_pack() for p in self.arena.params[i0:i1] if hasattr(p, "_ddp_amd_pack")]
        if descs and self.arena.data.is_cuda:
            from ..ops.common import native, stream_handle
            native().pack_conv_weights(descs, stream.cuda_stream if stream is not None
                                       else stream_handle())

    def zero_grad(self, set_to_none=False):
        if self._fused:
            self.arena.zero_grad()  # kernels accumulate into the arena: always zero, never None
        else:
            super().zero_grad(set_to_none=set_to_none)

    @torch.no_grad()
    def step(self, closure=None, zero_grad=False, counter=None, skip=None, params=None,
             stream=None, fused_taken=False, signal=None, lr_advance=None, norm_done=False):
        """One fused launch. ``params = (i0, i1)``: only parameters i0 <= i < i1 (arena order);
        ``stream``: launch on this torch stream instead of the current one. ``zero_grad=True`` also clears every gradient after its use (the
        next step then needs no zero_grad fill); ``counter=(int32 device ptr, delta)`` is
        advanced by the same launch (the on-device data cursor of engine/step.py); ``skip`` =
        device pointer of a uint32 error word: the update is skipped when it is non-zero.
        ``fused_taken=True``: skip the parameters whose update the backward already applied
        (register_in_backward). ``signal = (ticket ptr, flag ptr)``: the launch's last block to
        finish release-increments the uint32 flag (zeroed uint32 ticket). ``lr_advance``: this
        launch ends the training step, so an attached schedule moves on to the next step after
        it (default: a whole-arena step does, a ``params`` range does not — the pipelined step
        passes it for its last bucket). True: the launch stages the next step and a one-thread
        launch behind it makes it current; ``"stage"``: the caller's next batch launch does that
        (``DeviceLoader.fill(lr_sched=...)``: no extra dispatch in an engine step).
        With the gradient guard the sum-of-squares launch over ``params`` runs first;
        ``norm_done=True``: the caller already ran ``grad_sumsq`` over every parameter (the
        update always sums the partials of the WHOLE arena). A skipped step is counted by the
        launch that ends the step (``lr_advance``)."""
        if lr_advance is None:
            lr_advance = params is None
        if not self._fused:
            self._cpu_lr()
            if self.guarded:
                if closure is not None:  # the gradients come first
                    with torch.enable_grad():
                        loss = closure()
                    closure = lambda: loss  # noqa: E731
                c, skipped = self._cpu_guard(lr_advance)
                if skipped:
                    out = closure() if closure is not None else None
                    if lr_advance:
                        self.count_step()
                    if zero_grad:
                        super().zero_grad(set_to_none=False)
                    return out
                self._cpu_scale_grads(c)
            out = self._cpu_masked_step(closure) if self._no_decay else super().step(closure)
            self._cpu_ema()
            if lr_advance:
                self.count_step()
            if zero_grad:
                super().zero_grad(set_to_none=False)
            return out
        from ..ops.common import native, stream_handle
        s = stream.cuda_stream if stream is not None else stream_handle()
        exclude = pack_only = frozenset()
        if fused_taken:
            if self.guarded:
                raise RuntimeError("gradient guard: no update is taken in the backward")
            if self.updates_in_launch_only:
                raise RuntimeError(self.launch_only_reason + ": no update is taken in the "
                                   "backward")
            pack_only = self._master_in_backward()
            exclude = self._fused_in_backward() | pack_only
        items, n_items, descs = self._work_table(params, exclude, pack_only)
        sched = self._sched_kw(lr_advance)
        if self.guarded and not norm_done:
            self.grad_sumsq(params, stream)
        if n_items == 0:  # every tensor was updated in the backward: only the data cursor
            if sched.get("sched_advance"):
                native().counter_add(int(counter[0]) if counter else 0,
                                     int(counter[1]) if counter else 0, s,
                                     sched=sched["sched"], sched_mode=1)
                self.count_step()
            elif counter:
                native().counter_add(int(counter[0]), int(counter[1]), s)
            if signal:
                native().flag_signal(int(signal[1]), s)
            return None
        # one launch: SGD over every tensor + bf16 re-pack of every conv weight
        self._update_launch(items, n_items, s, descs=descs, zero_grad=zero_grad, counter=counter,
                            skip=skip, signal=signal, lr_advance=lr_advance)
        return None

    def state_dict(self):
        sd = super().state_dict()
        if self._schedule is not None:  # plain ints / floats / lists: loads with weights_only
            sd["lr_schedule"] = {"schedule": self._schedule.state_dict(), "step": self._lr_step}
        if self.guarded:
            sd["grad_guard"] = {"skipped": int(self.skipped_steps())}
        if self._fused:
            # expose the momentum buffers in torch.optim.SGD's per-parameter layout
            a = self.arena
            for i, p in enumerate(a.params):
                    sd["state"][i] = {"momentum_buffer": a.shaped(self.momentum_buffer, i).contiguous()}
        return sd

    def load_state_dict(self, sd):
        ls = sd.get("lr_schedule")
        if ls is not None:
            self.set_schedule(LRSchedule.from_state_dict(ls["schedule"]), step=int(ls["step"]))
        saved = sd["param_groups"][0] if sd.get("param_groups") else {}
        if "skip_nonfinite" in saved or "max_grad_norm" in saved:
            self._set_guard(saved.get("max_grad_norm"), saved.get("clip_eps", 1e-6),
                            saved.get("skip_nonfinite", False))
        gg = sd.get("grad_guard")
        if gg is not None and self.guarded:
            if self._guard_dev is not None:
                self._guard_dev.view(torch.int32)[2] = int(gg["skipped"])
            self._guard_cpu[2] = int(gg["skipped"])
        if "ema_decay" in saved:
            # the EMA is switched on with the saved decay and seeded from the masters as they
            # are; its contents travel in the checkpoint (utils/misc.py ``ema_state_dict``)
            self.set_ema(saved["ema_decay"])
        if "no_decay" in saved:
            self.set_no_decay([int(i) for i in saved["no_decay"]])
        mask = self.param_groups[0].get("no_decay")  # (a state dict without the key: as constructed)
        if not self._fused:
            out = super().load_state_dict({k: v for k, v in sd.items()
                                           if k not in ("lr_schedule", "grad_guard")})
            if self._ema_decay is not None:  # (an EMA that the saved groups do not know stays on)
                self.param_groups[0]["ema_decay"] = self._ema_decay
            if mask is not None:
                self.param_groups[0]["no_decay"] = mask
            return out
        a = self.arena
        st = sd.get("state", {})
        for i, p in enumerate(a.params):
            buf = st.get(i, st.get(str(i), {})).get("momentum_buffer")
            if buf is not None:
                a.shaped(self.momentum_buffer, i).copy_(buf.reshape(p.shape))
        for k in ("lr", "momentum", "weight_decay", "nesterov"):
            if sd.get("param_groups"):
                self.param_groups[0][k] = sd["param_groups"][0].get(k, self.param_groups[0][k])
