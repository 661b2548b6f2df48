"""Two-rank Gloo worker of tests/test_soft_targets_cpu.py: part3's loop (DDP, train_model) for
three steps with label smoothing and mixup; returns the parameters and the lam of every step."""
import torch

from dist_helpers import _init

STEPS, E, ALPHA = 3, 0.1, 0.2


def soft_worker(rank, world, port, q, per_rank_batch):
    try:
        _init(rank, world, port)
        import torch.distributed as dist
        from ddp_amd.data import CPULoader, SyntheticCIFAR10
        from ddp_amd.engine import CrossEntropyLoss
        from ddp_amd.engine.trainer import train_model
        from ddp_amd.models import VGG11
        from ddp_amd.optim import FusedSGD
        from ddp_amd.parallel import DistributedDataParallel, TorchCommunicator, check_replicas
        torch.manual_seed(89395)
        model = DistributedDataParallel(VGG11(), TorchCommunicator(), bucket_cap_mb=4.0,
                                        first_bucket_cap_mb=1.0)
        opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
        ds = SyntheticCIFAR10(True, n=per_rank_batch * world * STEPS)
        loader = CPULoader(ds, per_rank_batch, num_replicas=world, rank=rank, mixup_alpha=ALPHA)
        recs = []

        class Sink:
            def log(self, **kw):
                recs.append(kw)
        stats = train_model(model, loader, opt, CrossEntropyLoss(label_smoothing=E), 0, "cpu",
                            log=lambda s: None, metrics=Sink())
        params = torch.cat([p.detach().reshape(-1).clone() for p in model.parameters()])
        consistent = check_replicas(model.arena, world)
        dist.destroy_process_group()
        q.put((rank, {"params": params.numpy(), "lam": [r["lam"] for r in recs],
                      "table": loader.lam_table.tolist(), "iters": len(stats["iter_ns"]),
                      "consistent": consistent}))
    except Exception:
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
        raise
