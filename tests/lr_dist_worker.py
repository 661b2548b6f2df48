"""Gloo worker of tests/test_lr_schedule_cpu.py: DDP strategy with a warm-up schedule attached
to the optimizer vs the host setting the learning rate by hand every step."""
import torch

from dist_helpers import _init


def schedule_kwargs():
    return dict(base_lr=0.05, total_steps=4, warmup_steps=2, warmup_start_factor=0.1,
                decay="cosine")


def ddp_schedule_worker(rank, world, port, q, steps, per_rank_batch):
    try:
        _init(rank, world, port)
        import torch.distributed as dist
        from ddp_amd.models import VGG11
        from ddp_amd.optim import FusedSGD, LRSchedule
        from ddp_amd.parallel import TorchCommunicator, DistributedDataParallel, check_replicas
        from ddp_amd.engine import CrossEntropyLoss
        from ddp_amd.data import SyntheticCIFAR10, CPULoader
        sched = LRSchedule(**schedule_kwargs())
        table = sched.table()
        out = {}
        for mode in ("schedule", "by_hand"):
            torch.manual_seed(89395)
            comm = TorchCommunicator()
            model = DistributedDataParallel(VGG11(), comm, bucket_cap_mb=4.0,
                                            first_bucket_cap_mb=1.0)
            opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
            if mode == "schedule":
                opt.set_schedule(sched)
            crit = CrossEntropyLoss()
            loader = CPULoader(SyntheticCIFAR10(True, n=per_rank_batch * world * steps),
                               per_rank_batch, num_replicas=world, rank=rank)
            lrs = []
            for i, (x, y) in enumerate(loader):
                if i >= steps:
                    break
                if mode == "by_hand":
                    opt.param_groups[0]["lr"] = float(table[min(i, len(table) - 1)])
                lrs.append(opt.current_lr())
                opt.zero_grad()
                crit(model(x), y).backward()
                opt.step()
            out[mode] = torch.cat([p.detach().reshape(-1).clone()
                                   for p in model.parameters()]).numpy()
            out[mode + "_lrs"] = lrs
            out[mode + "_consistent"] = check_replicas(model.arena, world)
            out[mode + "_lr_step"] = opt.lr_step
        dist.destroy_process_group()
        q.put((rank, out))
    except Exception:
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
        raise
