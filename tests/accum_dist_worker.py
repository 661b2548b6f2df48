"""Two-rank Gloo worker of tests/test_accum_dist_cpu.py: train_model(accum_steps=2) over two
optimizer steps (four batches per rank) with DDP or a 2A / 2B strategy, counting bucket launches
and sync calls, next to a hand-accumulated local gradient of the first step."""
import copy

import torch

from dist_helpers import _init

K, STEPS = 2, 2


def accum_worker(rank, world, port, q, strategy, per_rank_batch, bucket_mb):
    try:
        _init(rank, world, port)
        import torch.distributed as dist
        from ddp_amd.data import CPULoader, SyntheticCIFAR10
        from ddp_amd.engine import CrossEntropyLoss
        from ddp_amd.engine.trainer import train_model
        from ddp_amd.models import VGG11
        from ddp_amd.optim import FusedSGD
        from ddp_amd.parallel import (STRATEGIES, DistributedDataParallel, TorchCommunicator,
                                      check_replicas)
        torch.manual_seed(89395)
        model = VGG11()
        plain = copy.deepcopy(model)
        comm = TorchCommunicator()
        counts = {"bucket_launches": 0, "syncs": 0, "buffer_syncs": 0}
        sync = None
        if strategy == "ddp":
            model = DistributedDataParallel(model, comm, bucket_cap_mb=bucket_mb,
                                            first_bucket_cap_mb=min(bucket_mb, 1.0))
            launch = model.reducer._launch

            def counted(b):
                counts["bucket_launches"] += 1
                launch(b)
            model.reducer._launch = counted
            sync_buffers = model._sync_buffers

            def counted_buffers():
                if getattr(model, "_buffer_sync_enabled", True):
                    counts["buffer_syncs"] += 1
                sync_buffers()
            model._sync_buffers = counted_buffers
        else:
            def sync(m):
                counts["syncs"] += 1
                STRATEGIES[strategy](m, comm)
        opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
        crit = CrossEntropyLoss()
        ds = SyntheticCIFAR10(True, n=per_rank_batch * world * K * STEPS)
        loader = CPULoader(ds, per_rank_batch, num_replicas=world, rank=rank)
        first = []
        step = opt.step

        def recording_step(*a, **kw):
            if not first:
                first.append(torch.cat([p.grad.reshape(-1).clone() for p in model.parameters()]))
            return step(*a, **kw)
        opt.step = recording_step
        stats = train_model(model, loader, opt, crit, 0, "cpu", sync, log=lambda s: None,
                            accum_steps=K)
        # the first optimizer step by hand on an unwrapped copy: accumulate locally, then average
        batches = [b for _, b in zip(range(K), CPULoader(ds, per_rank_batch, num_replicas=world,
                                                         rank=rank))]
        for x, y in batches:
            (crit(plain(x), y) / K).backward()
        local = torch.cat([p.grad.reshape(-1).clone() for p in plain.parameters()])
        mean = local.clone()
        dist.all_reduce(mean)
        mean /= world
        params = torch.cat([p.detach().reshape(-1).clone() for p in model.parameters()])
        info = {}
        if strategy == "ddp":
            info = {"consistent": check_replicas(model.arena, world),
                    "n_buckets": len(model.buckets)}
        dist.destroy_process_group()
        q.put((rank, {"params": params.numpy(), "grads0": first[0].numpy(), "mean": mean.numpy(),
                      "local": local.numpy(), "iters": len(stats["iter_ns"]), **counts, **info}))
    except Exception:
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
        raise
