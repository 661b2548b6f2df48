"""Gloo worker of tests/test_ema_cpu.py: DDP steps with the weight EMA on every rank. The EMA is
switched on after the wrapper's rank-0 broadcast, so it starts from the same weights everywhere,
and every rank averages the same masters."""
import torch

from dist_helpers import _init


def ddp_ema_worker(rank, world, port, q, steps, per_rank_batch, decay):
    try:
        _init(rank, world, port)
        import torch.distributed as dist
        from ddp_amd.models import VGG11
        from ddp_amd.optim import FusedSGD
        from ddp_amd.parallel import TorchCommunicator, DistributedDataParallel, check_replicas
        from ddp_amd.engine import CrossEntropyLoss
        from ddp_amd.data import SyntheticCIFAR10, CPULoader
        torch.manual_seed(89395 + rank)  # different initial weights: the broadcast makes them one
        comm = TorchCommunicator()
        model = DistributedDataParallel(VGG11(), comm, bucket_cap_mb=4.0, first_bucket_cap_mb=1.0)
        opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
        opt.set_ema(decay)
        flat = lambda: torch.cat([p.detach().reshape(-1).clone() for p in model.parameters()])
        snaps = [flat()]
        crit = CrossEntropyLoss()
        loader = CPULoader(SyntheticCIFAR10(True, n=per_rank_batch * world * steps),
                           per_rank_batch, num_replicas=world, rank=rank)
        for i, (x, y) in enumerate(loader):
            if i >= steps:
                break
            opt.zero_grad()
            crit(model(x), y).backward()
            opt.step()
            snaps.append(flat())
        ema = torch.cat([v.reshape(-1) for v in opt.ema_state().values()])
        out = {"ema": ema.numpy(), "snaps": torch.stack(snaps).numpy(),
               "consistent": check_replicas(model.arena, world)}
        dist.destroy_process_group()
        q.put((rank, out))
    except Exception:
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
        raise
