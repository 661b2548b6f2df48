"""Training and evaluation loops with the reference's observable behaviour.

Reference parity: ``train_model`` (part1/main.py:52-93; part2/part2a/main.py:118-160 with the
sync call at :143) and ``test_model`` (part1/main.py:96-111):
* per batch: timer start -> ``.to(device)`` -> zero_grad -> forward -> loss -> backward ->
  [gradient sync] -> step -> ``loss.item()``;
* ``[epoch, batch] loss: x.xxx`` every 20 batches (rank-local running mean, not all-reduced);
* iteration 0 is warm-up; the wall time of iterations 1..39 is summed and printed at 39;
* eval: model.eval(), no_grad, sum of per-batch mean CE divided by the NUMBER OF BATCHES,
  argmax accuracy over the whole (unsharded) test set, reference print format.
"""
import contextlib
import time

import torch
import torch.nn as nn

from ..utils.misc import fault_point
from ..utils.trace import trace_range


class CrossEntropyLoss(nn.Module):
    """``nn.CrossEntropyLoss()`` (mean); GPU logits use the fused softmax-CE HIP kernel.
    ``label_smoothing`` = E as in torch (0: the reference's loss); ``mix`` = (partner labels,
    lam) of a mixup batch (the loader's ``soft_targets()``): lam * CE(target) + (1 - lam) *
    CE(partner). Both go through the soft-target form of the same kernels (``soft``)."""

    def __init__(self, label_smoothing=0.0):
        super().__init__()
        e = float(label_smoothing)
        if not 0.0 <= e < 1.0:
            raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing}")
        self.label_smoothing = e

    def soft(self, mix=None):
        """The SoftTarget of a batch (ops/common.py), or None for the plain one-hot loss."""
        if not self.label_smoothing and mix is None:
            return None
        from ..ops.common import SoftTarget
        return SoftTarget(self.label_smoothing, *(mix or (None, None)))

    def forward(self, logits, target, mix=None):
        soft = self.soft(mix)
        if logits.is_cuda:
            from ..ops.layers import cross_entropy
            return cross_entropy(logits, target, soft)
        if soft is not None:
            return soft.torch_loss(logits, target)
        return nn.functional.cross_entropy(logits, target)


def batch_mix(loader):
    """(partner labels, lam) of the mixup batch a loader produced last, or None."""
    return loader.soft_targets() if hasattr(loader, "soft_targets") else None


def _scheduled_lr(optimizer):
    """Extra metrics field of one iteration: the learning rate it runs with, only when a
    schedule is attached (optim/sgd.py set_schedule; read from the host mirror, no sync)."""
    if getattr(optimizer, "schedule", None) is None:
        return {}
    return {"lr": optimizer.current_lr()}


def _guard_stats(optimizer):
    """Extra metrics fields of one iteration with the optimizer's gradient guard on (optim/sgd.py
    max_grad_norm / skip_nonfinite): the gradient norm, the clip coefficient and the skipped
    steps so far. Device reads: call after the iteration's synchronize."""
    if not getattr(optimizer, "guarded", False):
        return {}
    return {"grad_norm": float(optimizer.grad_norm()), "clip_coef": float(optimizer.clip_coef()),
            "skipped": int(optimizer.skipped_steps())}


def _ema_field(optimizer):
    """Extra metrics field of one iteration with the optimizer's weight EMA on (set_ema)."""
    d = getattr(optimizer, "ema_decay", None)
    return {} if d is None else {"ema_decay": d}


def _optimizer_field(optimizer):
    """Extra metrics field of one iteration: the optimizer's name where it is not the reference's
    SGD family (optim/adamw.py ``metrics_name``; records of sgd and lars runs stay as they were)."""
    name = getattr(optimizer, "metrics_name", None)
    mask = getattr(optimizer, "no_decay_name", None)  # --no-decay-1d: "1d"
    return {**({} if name is None else {"optimizer": name}),
            **({} if mask is None else {"no_decay": mask})}


def micro_batch_ctx(model, first, last):
    """DDP wrapper state of one micro-batch of an accumulated step: no gradient collective
    before the last one (``no_sync``), the buffer broadcast only before the first one."""
    st = contextlib.ExitStack()
    if not last and hasattr(model, "no_sync"):
        st.enter_context(model.no_sync())
    if not first and hasattr(model, "no_buffer_sync"):
        st.enter_context(model.no_buffer_sync())
    return st


def _groups(loader, k):
    """The loader's batches in groups of ``k`` (the last group may be shorter), each as
    (data, target, mix) with ``mix`` = the batch's mixup partner labels and lam, or None."""
    group = []
    for data, target in loader:
        group.append((data, target, batch_mix(loader)))
        if len(group) == k:
            yield group
            group = []
    if group:
        yield group


@contextlib.contextmanager
def grad_scaled(optimizer, m):
    """The optimizer's grad_scale set, for the launches issued inside (a launch argument: baked
    into a capture), to that of the update that consumes the sum of ``m`` micro-batch
    gradients: float32(grad_scale / m), rounded on the host — the value every update site
    multiplies the accumulated gradient by (exact for m a power of two). m == 1 touches
    nothing."""
    if m == 1:
        yield
        return
    base = optimizer.grad_scale_factor
    optimizer.grad_scale_factor = float(torch.tensor(float(base) / m, dtype=torch.float32))
    try:
        yield
    finally:
        optimizer.grad_scale_factor = base


class _Iterations:
    """Per-iteration bookkeeping of both loops (an iteration is one optimizer step): the timer,
    the ``[epoch, batch] loss`` line every 20 iterations, the 1..39 window and its two prints,
    the metrics record (``accum`` only with accumulation), the watchdog beat, ``stats``."""

    def __init__(self, optimizer, epoch, rank, log, metrics, watchdog, accum_steps):
        self.optimizer, self.epoch, self.rank, self.log = optimizer, epoch, rank, log
        self.metrics, self.watchdog, self.accum = metrics, watchdog, accum_steps > 1
        self.stats = {"iter_ns": [], "total_1_39_ns": 0}

    def begin(self, it):
        fault_point(self.rank, it)
        self.start = time.perf_counter_ns()
        self.lr = _scheduled_lr(self.optimizer)

    def end(self, it, m, mean_loss, lam=None):
        """``mean_loss()``: the value of the loss line, asked for when one is due; returns
        whether it was (the caller then starts its running mean anew). ``lam``: with mixup the
        mixing weights of the iteration's micro-batches (a list with accumulation)."""
        due = it % 20 == 19
        if due:
            self.log(f'[{self.epoch + 1}, {it + 1:5d}] loss: {mean_loss():.3f}')
        dt = time.perf_counter_ns() - self.start
        st = self.stats
        st["iter_ns"].append(dt)
        if 0 < it < 40:
            st["total_1_39_ns"] += dt
        if it == 39:
            self.log(f'Total time for 1-39 iteration in ns: {st["total_1_39_ns"]}')
            self.log(f'Average time for 1-39 iteration in ns: {st["total_1_39_ns"] / 39.0}')
        if self.metrics is not None:
            self.metrics.log(event="iter", epoch=self.epoch, batch=it, ns=dt,
                             **({"accum": m} if self.accum else {}), **self.lr,
                             **_guard_stats(self.optimizer), **_ema_field(self.optimizer),
                             **_optimizer_field(self.optimizer),
                             **({"lam": lam if self.accum else lam[0]} if lam else {}))
        if self.watchdog is not None:
            self.watchdog.beat()
        return due


def train_model(model, train_loader, optimizer, criterion, epoch, device="cpu", sync=None,
                log=print, metrics=None, watchdog=None, rank=0, accum_steps=1):
    """An iteration is one optimizer step over up to ``accum_steps`` consecutive batches (1: the
    reference's loop; the epoch's last group may hold fewer, m), with the gradient sync (DDP
    buckets, 2A/2B) once, after the last micro-batch. Where the 1/m goes:
    the fused optimizer of the GPU takes it as float32(grad_scale / m) in its update launch, as
    the captured steps do (the micro-batch gradients are the plain ones: scaling the loss would
    round every bf16 activation gradient differently when m is no power of two); every other
    optimizer path (torch.optim.SGD on the CPU ignores grad_scale) gets each backward on
    loss / m. The losses are read after the step (the reference's order: one host
    synchronisation per iteration)."""
    fused = bool(getattr(optimizer, "_fused", False)) and hasattr(optimizer, "grad_scale_factor")
    book = _Iterations(optimizer, epoch, rank, log, metrics, watchdog, accum_steps)
    running_loss = 0.0
    for it, group in enumerate(_groups(train_loader, accum_steps)):
        book.begin(it)
        m = len(group)
        losses = []
        for j, (data, target, mix) in enumerate(group):
            with trace_range("data"):
                data, target = data.to(device), target.to(device)
            if j == 0:
                optimizer.zero_grad()
            with micro_batch_ctx(model, j == 0, j == m - 1):
                with trace_range("forward"):
                    output = model(data)
                    loss = criterion(output, target, mix) if mix else criterion(output, target)
                with trace_range("backward"):
                    (loss if fused or m == 1 else loss / m).backward()
            losses.append(loss.detach())
        if sync is not None:
            with trace_range("sync"):
                sync(model)
        with trace_range("optimizer"), grad_scaled(optimizer, m if fused else 1):
            optimizer.step()

        running_loss += sum(v.item() for v in losses) / m
        lam = [float(mix[1]) for _, _, mix in group if mix] if metrics is not None else None
        if book.end(it, m, lambda: running_loss / 20, lam):
            running_loss = 0.0
    return book.stats


def train_model_graph(step, train_loader, epoch, log=print, metrics=None, watchdog=None, rank=0,
                      accum_steps=1):
    """``train_model`` over a captured TrainStep (engine/step.py): every iteration is ONE graph
    replay (augment + forward + backward + sync + optimizer) followed by a device synchronize,
    so the per-iteration timer keeps the reference's meaning (the reference's ``loss.item()``
    synchronises each iteration too). The loss print every 20 batches reads the device loss
    accumulator (same running mean as the reference).

    The captured step has a fixed batch shape, so only the floor(L/B) FULL batches of the shard
    are replays; a partial last batch (L % B samples, e.g. 80 of 50 000 at B = 256) runs as one
    eager step on exactly those samples (``TrainStep.tail_step``) — the same samples and the
    same partial-batch mean as the eager loop and the reference's DataLoader.

    ``accum_steps`` = K > 1 (the step was built with the same K): an iteration is one optimizer
    step — a replay over K batches, or at the end of the epoch ONE eager step over the leftover
    full batches and the partial batch (``accum_epoch_plan``; with K = 1 that is
    ``graph_epoch_plan``: the partial batch alone)."""
    K = accum_steps
    if getattr(step, "accum_steps", 1) != K:
        raise ValueError(f"the step accumulates {getattr(step, 'accum_steps', 1)} micro-batches, "
                         f"the loop was asked for {K}")
    book = _Iterations(step.optimizer, epoch, rank, log, metrics, watchdog, K)
    L, B = train_loader.idx.numel(), train_loader.batch_size
    replays, left, tail = accum_epoch_plan(L, B, K, train_loader.max_batches)
    sizes = [B] * left + ([tail] if tail else [])  # the epoch's last, eager step
    step.pop_loss()
    micro = 0  # micro-batches in the loss meter since the last print
    for it in range(replays + (1 if sizes else 0)):
        book.begin(it)
        if it < replays:
            step.step()
            m = K
        else:
            m = len(sizes)
            step.tail_step([(*train_loader.batch((replays * K + j) * B, n),
                             batch_mix(train_loader)) for j, n in enumerate(sizes)])
        micro += m
        torch.cuda.synchronize()
        lam = step.lams() if metrics is not None and hasattr(step, "lams") else None
        if book.end(it, m, lambda: step.pop_loss() / micro, lam):
            micro = 0
    if hasattr(step, "check_error"):
        step.check_error()
    book.stats["graph_replays"] = replays
    return book.stats


def accum_epoch_plan(n_samples, batch, K, max_batches=None):
    """(replayed optimizer steps, leftover full micro-batches, tail size) of one --graph epoch
    with --accum-steps K over a shard of ``n_samples``: of the nfull full batches (at most
    ``max_batches`` loader batches in all) floor(nfull / K) groups are replays; the
    nfull mod K leftover full batches and the partial batch, if the epoch reaches it, form ONE
    eager optimizer step."""
    nfull, tail = graph_epoch_plan(n_samples, batch, max_batches)
    return nfull // K, nfull % K, tail


def graph_epoch_plan(n_samples, batch_size, max_batches=None):
    """(replayed full batches, eager tail size) of one --graph epoch over a shard of
    ``n_samples`` — the CPU-checkable schedule ``train_model_graph`` follows."""
    nb = -(-n_samples // batch_size)
    if max_batches:
        nb = min(nb, max_batches)
    nfull = min(nb, n_samples // batch_size)
    tail = n_samples - nfull * batch_size if nb > nfull else 0
    return nfull, tail


def test_model(model, test_loader, criterion, device="cpu", log=print, watchdog=None, tag=""):
    """``tag``: appended to ``Test set`` in the result line (`` (EMA)``: the pass on the
    averaged weights, engine/apps.py); empty: the reference's line."""
    model.eval()
    test_loss = 0
    correct = 0
    nb = 0
    inner = getattr(model, "module", model)
    fused = (torch.device(device).type == "cuda" and hasattr(inner, "forward_metrics")
             and type(criterion) is CrossEntropyLoss)
    if type(criterion) is CrossEntropyLoss:
        criterion = CrossEntropyLoss()  # evaluation is the plain loss: no smoothing, no mixup
    if fused:  # loss + argmax hits accumulated on the device by the classifier kernel
        loss_acc = torch.zeros((), dtype=torch.float32, device=device)
        hits = torch.zeros((), dtype=torch.int32, device=device)
    with torch.no_grad():
        for data, target in test_loader:
            data, target = data.to(device), target.to(device)
            if fused:
                inner.forward_metrics(data, target, loss_acc, hits)
            else:
                output = model(data)
                test_loss += criterion(output, target)
                pred = output.max(1, keepdim=True)[1]
                correct += pred.eq(target.view_as(pred)).sum().item()
            nb += 1
            if watchdog is not None:
                watchdog.beat()
    if fused:
        test_loss, correct = float(loss_acc), int(hits)
    n = len(test_loader.dataset)
    test_loss = float(test_loss) / max(nb, 1)
    log('Test set{}: Average loss: {:.4f}, Accuracy: {}/{} ({:.0f}%)\n'.format(
        tag, test_loss, correct, n, 100. * correct / n))
    model.train()
    return test_loss, correct
