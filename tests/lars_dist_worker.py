"""Gloo worker of tests/test_lars_cpu.py: DDP steps with the LARS optimizer on every rank, and
the sharded (ZeRO-1) update, which has no whole tensor to take a norm of and must refuse it."""
import torch

from dist_helpers import _init


def ddp_lars_worker(rank, world, port, q, steps, per_rank_batch):
    try:
        _init(rank, world, port)
        import torch.distributed as dist
        from ddp_amd.models import VGG11
        from ddp_amd.optim import LARS
        from ddp_amd.parallel import TorchCommunicator, DistributedDataParallel, check_replicas
        from ddp_amd.parallel.zero import ShardedUpdate, arena_buckets
        from ddp_amd.engine import CrossEntropyLoss
        from ddp_amd.data import SyntheticCIFAR10, CPULoader
        torch.manual_seed(89395)
        comm = TorchCommunicator()
        model = DistributedDataParallel(VGG11(), comm, bucket_cap_mb=4.0, first_bucket_cap_mb=1.0)
        opt = LARS(model.parameters(), lr=0.4, momentum=0.9, weight_decay=1e-4,
                   trust_coefficient=0.02)
        start = torch.cat([p.detach().reshape(-1).clone() for p in model.parameters()])
        crit = CrossEntropyLoss()
        loader = CPULoader(SyntheticCIFAR10(True, n=per_rank_batch * world * steps),
                           per_rank_batch, num_replicas=world, rank=rank)
        for i, (x, y) in enumerate(loader):
            if i >= steps:
                break
            opt.zero_grad()
            crit(model(x), y).backward()
            opt.step()
        out = {"params": torch.cat([p.detach().reshape(-1).clone()
                                    for p in model.parameters()]).numpy(),
               "moved": bool((start != torch.cat([p.detach().reshape(-1)
                                                  for p in model.parameters()])).any()),
               "trust": opt.trust_ratios().clone().numpy(),
               "dims": [p.dim() for p in model.parameters()],
               "consistent": check_replicas(model.arena, world)}
        # the sharded update: refused where it is built and where it would run
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
