"""Gloo worker of tests/test_lamb_cpu.py: steps with LAMB on every rank under one gradient-sync
strategy -- ``ddp`` (the bucketed wrapper), ``gather_scatter`` (part 2A) or ``allreduce`` (part
2B) -- on tests/adamw_dist_worker.py's model without BatchNorm (the mean of the ranks' gradients
is then the gradient of the concatenated batch)."""
import torch

from adamw_dist_worker import batch, model  # noqa: F401  (re-exported for the test)
from dist_helpers import _init


def lamb_worker(rank, world, port, q, strategy, steps, per_rank_batch):
    try:
        _init(rank, world, port)
        import torch.distributed as dist
        from ddp_amd.optim import LAMB
        from ddp_amd.parallel import (STRATEGIES, TorchCommunicator, DistributedDataParallel,
                                      check_replicas)
        comm = TorchCommunicator()
        net = model()
        if strategy == "ddp":
            net = DistributedDataParallel(net, comm, bucket_cap_mb=0.001,
                                          first_bucket_cap_mb=0.001)
        opt = LAMB(net.parameters(), lr=2e-3)
        for s in range(steps):
            x, y = batch(s, rank, per_rank_batch)
            opt.zero_grad()
            torch.nn.functional.cross_entropy(net(x), y).backward()
            if strategy != "ddp":
                STRATEGIES[strategy](net, comm)
            opt.step()
        params = torch.cat([p.detach().reshape(-1).clone() for p in net.parameters()])
        out = {"params": params.numpy(), "trust": opt.trust_ratios().clone().numpy(),
               "t": opt.lr_step}
        if strategy == "ddp":
            out["n_buckets"] = len(net.buckets)
            out["consistent"] = check_replicas(net.arena, world)
        dist.destroy_process_group()
        q.put((rank, out))
    except Exception:
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
        raise
