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
    """``nn.CrossEntropyLoss()`` (mean); GPU logits use the fused softmax-CE HIP kernel."""

    def forward(self, logits, target):
        if logits.is_cuda:
            from ..ops.layers import cross_entropy
            return cross_entropy(logits, target)
        return nn.functional.cross_entropy(logits, target)


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
    """The loader's batches in groups of ``k`` (the last group may be shorter)."""
    group = []
    for item in loader:
        group.append(item)
        if len(group) == k:
            yield group
            group = []
    if group:
        yield group


def _train_model_accum(model, train_loader, optimizer, criterion, epoch, device, sync, log,
                       metrics, watchdog, rank, accum_steps):
    """``train_model`` with gradient accumulation: an iteration is one optimizer step over up
    to ``accum_steps`` consecutive batches (the epoch's last group may hold fewer, m), each
    the gradient sync (DDP buckets, 2A/2B) once, after the last micro-batch. Where the 1/m goes:
    the fused optimizer of the GPU takes it as float32(grad_scale / m) in its update launch, as
    the captured steps do (the micro-batch gradients are the plain ones: scaling the loss would
    round every bf16 activation gradient differently when m is no power of two); every other
    optimizer path (torch.optim.SGD on the CPU ignores grad_scale) gets each backward on
    loss / m."""
    fused = bool(getattr(optimizer, "_fused", False)) and hasattr(optimizer, "grad_scale_factor")
    running_loss = 0.0
    total_time = 0
    stats = {"iter_ns": []}
    for it, group in enumerate(_groups(train_loader, accum_steps)):
        fault_point(rank, it)
        start_time = time.perf_counter_ns()
        lr = _scheduled_lr(optimizer)
        m = len(group)
        optimizer.zero_grad()
        loss_sum = 0.0
        for j, (data, target) in enumerate(group):
            with trace_range("data"):
                data, target = data.to(device), target.to(device)
            with micro_batch_ctx(model, j == 0, j == m - 1):
                with trace_range("forward"):
                    output = model(data)
                    loss = criterion(output, target)
                with trace_range("backward"):
                    (loss if fused else loss / m).backward()
            loss_sum += loss.item()
        if sync is not None:
            with trace_range("sync"):
                sync(model)
        with trace_range("optimizer"):
            if fused and m > 1:
                base = optimizer.grad_scale_factor
                optimizer.grad_scale_factor = float(torch.tensor(float(base) / m,
                                                                 dtype=torch.float32))
                try:
                    optimizer.step()
                finally:
                    optimizer.grad_scale_factor = base
            else:
                optimizer.step()

        running_loss += loss_sum / m
        if it % 20 == 19:
            log(f'[{epoch + 1}, {it + 1:5d}] loss: {running_loss / 20:.3f}')
            running_loss = 0.0

        dt = time.perf_counter_ns() - start_time
        stats["iter_ns"].append(dt)
        if 0 < it < 40:
            total_time += dt
        if it == 39:
            log(f'Total time for 1-39 iteration in ns: {total_time}')
            log(f'Average time for 1-39 iteration in ns: {total_time / 39.0}')
        if metrics is not None:
            metrics.log(event="iter", epoch=epoch, batch=it, ns=dt, accum=m, **lr,
                        **_guard_stats(optimizer))
        if watchdog is not None:
            watchdog.beat()
    stats["total_1_39_ns"] = total_time
    return stats


def train_model(model, train_loader, optimizer, criterion, epoch, device="cpu", sync=None,
                log=print, metrics=None, watchdog=None, rank=0, accum_steps=1):
    if accum_steps > 1:
        return _train_model_accum(model, train_loader, optimizer, criterion, epoch, device,
                                  sync, log, metrics, watchdog, rank, accum_steps)
    running_loss = 0.0
    total_time = 0
    stats = {"iter_ns": []}
    for batch_idx, (data, target) in enumerate(train_loader):
        fault_point(rank, batch_idx)
        start_time = time.perf_counter_ns()
        lr = _scheduled_lr(optimizer)
        with trace_range("data"):
            data, target = data.to(device), target.to(device)

        optimizer.zero_grad()
        with trace_range("forward"):
            output = model(data)
            loss = criterion(output, target)
        with trace_range("backward"):
            loss.backward()
        if sync is not None:
            with trace_range("sync"):
                sync(model)
        with trace_range("optimizer"):
            optimizer.step()

        running_loss += loss.item()
        if batch_idx % 20 == 19:
            log(f'[{epoch + 1}, {batch_idx + 1:5d}] loss: {running_loss / 20:.3f}')
            running_loss = 0.0

        dt = time.perf_counter_ns() - start_time
        stats["iter_ns"].append(dt)
        if 0 < batch_idx < 40:
            total_time += dt
        if batch_idx == 39:
            log(f'Total time for 1-39 iteration in ns: {total_time}')
            log(f'Average time for 1-39 iteration in ns: {total_time / 39.0}')
        if metrics is not None:
            metrics.log(event="iter", epoch=epoch, batch=batch_idx, ns=dt, **lr,
                        **_guard_stats(optimizer))
        if watchdog is not None:
            watchdog.beat()
    stats["total_1_39_ns"] = total_time
    return stats


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
    full batches and the partial batch (``accum_epoch_plan``)."""
    if accum_steps > 1:
        return _train_model_graph_accum(step, train_loader, epoch, log, metrics, watchdog, rank,
                                        accum_steps)
    total_time = 0
    stats = {"iter_ns": []}
    nb = len(train_loader)
    L, B = train_loader.idx.numel(), train_loader.batch_size
    nfull = L // B
    step.pop_loss()
    for batch_idx in range(nb):
        fault_point(rank, batch_idx)
        start_time = time.perf_counter_ns()
        lr = _scheduled_lr(step.optimizer)
        if batch_idx < nfull:
            step.step()
        else:
            step.tail_step(*train_loader.batch(batch_idx * B, L - batch_idx * B))
        torch.cuda.synchronize()
        if batch_idx % 20 == 19:
            log(f'[{epoch + 1}, {batch_idx + 1:5d}] loss: {step.pop_loss() / 20:.3f}')
        dt = time.perf_counter_ns() - start_time
        stats["iter_ns"].append(dt)
        if 0 < batch_idx < 40:
            total_time += dt
        if batch_idx == 39:
            log(f'Total time for 1-39 iteration in ns: {total_time}')
            log(f'Average time for 1-39 iteration in ns: {total_time / 39.0}')
        if metrics is not None:
            metrics.log(event="iter", epoch=epoch, batch=batch_idx, ns=dt, **lr,
                        **_guard_stats(step.optimizer))
        if watchdog is not None:
            watchdog.beat()
    if hasattr(step, "check_error"):
        step.check_error()
    stats["total_1_39_ns"] = total_time
    stats["graph_replays"] = min(nb, nfull)
    return stats


def _train_model_graph_accum(step, train_loader, epoch, log, metrics, watchdog, rank, K):
    if getattr(step, "accum_steps", 1) != K:
        raise ValueError(f"the step accumulates {getattr(step, 'accum_steps', 1)} micro-batches, "
                         f"the loop was asked for {K}")
    total_time = 0
    stats = {"iter_ns": []}
    L, B = train_loader.idx.numel(), train_loader.batch_size
    replays, left, tail = accum_epoch_plan(L, B, K, train_loader.max_batches)
    n_iter = replays + (1 if left or tail else 0)
    step.pop_loss()
    micro = 0  # micro-batches in the loss meter since the last print
    for it in range(n_iter):
        fault_point(rank, it)
        start_time = time.perf_counter_ns()
        lr = _scheduled_lr(step.optimizer)
        if it < replays:
            step.step()
            m = K
        else:
            first = replays * K
            sizes = [B] * left + ([tail] if tail else [])
            m = len(sizes)
            step.tail_step([train_loader.batch((first + j) * B, n) for j, n in enumerate(sizes)])
        micro += m
        torch.cuda.synchronize()
        if it % 20 == 19:
            log(f'[{epoch + 1}, {it + 1:5d}] loss: {step.pop_loss() / micro:.3f}')
            micro = 0
        dt = time.perf_counter_ns() - start_time
        stats["iter_ns"].append(dt)
        if 0 < it < 40:
            total_time += dt
        if it == 39:
            log(f'Total time for 1-39 iteration in ns: {total_time}')
            log(f'Average time for 1-39 iteration in ns: {total_time / 39.0}')
        if metrics is not None:
            metrics.log(event="iter", epoch=epoch, batch=it, ns=dt, accum=m, **lr,
                        **_guard_stats(step.optimizer))
        if watchdog is not None:
            watchdog.beat()
    if hasattr(step, "check_error"):
        step.check_error()
    stats["total_1_39_ns"] = total_time
    stats["graph_replays"] = replays
    return stats


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


def test_model(model, test_loader, criterion, device="cpu", log=print, watchdog=None):
    model.eval()
    test_loss = 0
    correct = 0
    nb = 0
    inner = getattr(model, "module", model)
    fused = (torch.device(device).type == "cuda" and hasattr(inner, "forward_metrics")
             and type(criterion) is CrossEntropyLoss)
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
    log('Test set: Average loss: {:.4f}, Accuracy: {}/{} ({:.0f}%)\n'.format(
        test_loss, correct, n, 100. * correct / n))
    model.train()
    return test_loss, correct
