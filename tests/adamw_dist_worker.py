"""Gloo worker of tests/test_adamw_cpu.py: DDP steps with AdamW on every rank, on a model without
BatchNorm (the mean of the ranks' gradients is then the gradient of the concatenated batch)."""
import torch

from dist_helpers import _init


def model(seed=7):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 6, 3, padding=1), torch.nn.Tanh(),
                               torch.nn.Flatten(), torch.nn.Linear(6 * 8 * 8, 5))


def batch(step, rank, n):
    g = torch.Generator().manual_seed(1000 + 10 * step + rank)
    return torch.randn(n, 3, 8, 8, generator=g), torch.randint(0, 5, (n,), generator=g)


def ddp_adamw_worker(rank, world, port, q, steps, per_rank_batch):
    try:
        _init(rank, world, port)
        import torch.distributed as dist
        from ddp_amd.optim import AdamW
        from ddp_amd.parallel import TorchCommunicator, DistributedDataParallel, check_replicas
        comm = TorchCommunicator()
        ddp = DistributedDataParallel(model(), comm, bucket_cap_mb=0.001,
                                      first_bucket_cap_mb=0.001)
        opt = AdamW(ddp.parameters(), lr=1e-3)
        for s in range(steps):
            x, y = batch(s, rank, per_rank_batch)
            opt.zero_grad()
            torch.nn.functional.cross_entropy(ddp(x), y).backward()
            opt.step()
        params = torch.cat([p.detach().reshape(-1).clone() for p in ddp.parameters()])
        sd = opt.state_dict()
        v = torch.cat([sd["state"][i]["exp_avg_sq"].reshape(-1) for i in range(len(sd["state"]))])
        out = {"params": params.numpy(), "v": v.numpy(), "t": opt.lr_step,
               "n_buckets": len(ddp.buckets), "consistent": check_replicas(ddp.arena, world)}
        dist.destroy_process_group()
        q.put((rank, out))
    except Exception:
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
        raise
