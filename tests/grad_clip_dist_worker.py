"""Gloo worker of tests/test_grad_clip_cpu.py: DDP and part-2B (all-reduce) steps with gradient
clipping on every rank. The norm is that of the averaged gradient, so the replicas stay
identical and agree on it; the sharded (ZeRO-1) update has only a shard of the gradient and must
refuse such an optimizer."""
import torch

from dist_helpers import _init

MAX_NORM = 0.05  # far below VGG-11's gradient norm at initialisation: every step clips


def clip_worker(rank, world, port, q, strategy, steps, per_rank_batch):
    try:
        _init(rank, world, port)
        import torch.distributed as dist
        from ddp_amd.models import VGG11
        from ddp_amd.optim import FusedSGD
        from ddp_amd.parallel import (TorchCommunicator, DistributedDataParallel, STRATEGIES,
                                      check_replicas)
        from ddp_amd.parallel.zero import ShardedUpdate, arena_buckets
        from ddp_amd.engine import CrossEntropyLoss
        from ddp_amd.data import SyntheticCIFAR10, CPULoader
        torch.manual_seed(89395)
        comm = TorchCommunicator()
        model = VGG11()
        if strategy == "ddp":
            model = DistributedDataParallel(model, comm, bucket_cap_mb=4.0,
                                            first_bucket_cap_mb=1.0)
        opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4,
                       max_grad_norm=MAX_NORM, skip_nonfinite=True)
        crit = CrossEntropyLoss()
        loader = CPULoader(SyntheticCIFAR10(True, n=per_rank_batch * world * steps),
                           per_rank_batch, num_replicas=world, rank=rank)
        norms, coefs = [], []
        for i, (x, y) in enumerate(loader):
            if i >= steps:
                break
            opt.zero_grad()
            crit(model(x), y).backward()
            if strategy in STRATEGIES:
                STRATEGIES[strategy](model, comm)
            opt.step()
            norms.append(float(opt.grad_norm()))
            coefs.append(float(opt.clip_coef()))
        out = {"params": torch.cat([p.detach().reshape(-1).clone()
                                    for p in model.parameters()]).numpy(),
               "norms": norms, "coefs": coefs, "skipped": int(opt.skipped_steps())}
        if strategy == "ddp":
            out["consistent"] = check_replicas(model.arena, world)
            a = model.arena
            try:
                ShardedUpdate(a, opt, comm, arena_buckets(a, [len(a.params) // 2]))
                out["sharded"] = "built"
            except ValueError as e:
                out["sharded"] = str(e)
            try:
                opt.step_elements(0, 64)
                out["elements"] = "ran"
            except ValueError as e:
                out["elements"] = str(e)
        dist.destroy_process_group()
        q.put((rank, out))
    except Exception:
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
        raise
