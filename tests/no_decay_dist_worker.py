"""Gloo worker of tests/test_no_decay_cpu.py: the sharded updates (parallel/zero.py) under the
optimizer's no-decay mask against their replicated masked twins, after the workers of
tests/dist_helpers.py (``zero_worker``, ``shard16_worker``)."""
import torch

from dist_helpers import _init

LR, MOM, WD = 0.05, 0.9, 0.02


def sharded_worker(rank, world, port, q, mode, steps):
    """``mode`` "zero": FusedSGD(no_decay="1d").step() behind DDP's all-reduce vs ShardedUpdate;
    "shard16": the replicated update with the GPU's operand semantics (as ``shard16_worker``), wd
    per tensor, vs ShardedBf16Update. Three buckets; the LAST parameters' bucket starts at the
    last BatchNorm's gamma: {gamma, beta, classifier weight, classifier bias}, so at world 2 its
    shard boundary lies inside the classifier's weight."""
    try:
        _init(rank, world, port)
        import torch.distributed as dist
        from ddp_amd.data import CPULoader, SyntheticCIFAR10
        from ddp_amd.engine import CrossEntropyLoss
        from ddp_amd.models import VGG11
        from ddp_amd.optim import FusedSGD
        from ddp_amd.parallel import DistributedDataParallel, TorchCommunicator, check_replicas
        from ddp_amd.parallel.comm import AVG
        from ddp_amd.parallel.zero import (ShardedBf16Update, ShardedUpdate, arena_buckets,
                                           operand_tensors)
        comm = TorchCommunicator()
        crit = CrossEntropyLoss()
        loader = CPULoader(SyntheticCIFAR10(True, n=4 * world * steps), 4, num_replicas=world,
                           rank=rank)
        batches = [b for _, b in zip(range(steps), loader)]
        out = {}
        for arm in ("replicated", "replicated_all_decayed", "sharded"):
            torch.manual_seed(89395)
            ddp = DistributedDataParallel(VGG11(), comm, bucket_cap_mb=4.0)
            mask = None if arm == "replicated_all_decayed" else "1d"
            opt = FusedSGD(ddp.parameters(), lr=LR, momentum=MOM, weight_decay=WD, no_decay=mask)
            a = ddp.arena
            n = len(a.params)
            assert [p.dim() for p in a.params[n - 4:]] == [1, 1, 2, 1]
            pidx = {id(p): i for i, p in enumerate(a.params)}
            firsts = [pidx[id(ddp.module.layers[11].weight)], n - 4]
            buckets = arena_buckets(a, firsts)
            assert len(buckets) == 3 and buckets[0][0] == (n - 4, n)
            ends = list(a.offsets[1:]) + [a.total]
            nd = opt.no_decay_mask
            op = operand_tensors(a)
            upd = master = mom = None
            if arm == "sharded":
                cls = ShardedUpdate if mode == "zero" else ShardedBf16Update
                upd = cls(a, opt, comm, buckets)
                # every rank's shard of the small bucket holds a masked and an unmasked run
                mixed = []
                for r in range(world):
                    lo, hi = buckets[0][1]
                    per = (hi - lo) // world
                    s0, s1 = lo + r * per, lo + (r + 1) * per
                    kinds = {m for _, _, m in opt._decay_runs(s0, s1)}
                    mixed.append(kinds == {True, False})
                out["mixed_shards"] = mixed
            elif mode == "shard16":
                master, mom = a.data.detach().clone(), torch.zeros_like(a.data)

                def materialize():
                    with torch.no_grad():
                        for (o, e), is_op in zip(zip(a.offsets, ends), op):
                            a.data[o:e] = (master[o:e].to(torch.bfloat16).float() if is_op
                                           else master[o:e])
                materialize()
            for x, y in batches:
                opt.zero_grad()
                if upd is None and mode == "zero":
                    crit(ddp(x), y).backward()
                    opt.step()
                    continue
                with ddp.no_sync():
                    crit(ddp(x), y).backward()
                if upd is not None:
                    for j in range(len(buckets)):
                        upd.step(j)
                else:
                    with torch.no_grad():
                        comm.all_reduce(a.grad, AVG)
                        d = a.grad.clone()
                        for (o, e), masked in zip(zip(a.offsets, ends), nd):
                            if not masked:
                                d[o:e].add_(master[o:e], alpha=WD)
                        mom.mul_(MOM).add_(d)
                        master.add_(mom, alpha=-LR)
                        a.grad.zero_()
                    materialize()
            if upd is not None:
                out["grad_zero"] = bool((a.grad == 0).all())
                if mode == "shard16":
                    upd.gather_masters()
                    out[arm], out[arm + "_momentum"] = upd.master.clone(), upd.momentum.clone()
                else:
                    # the ZeRO-1 CPU path keeps its momentum flat, complete on the owner only
                    for (_, (lo, hi)) in buckets:
                        comm.all_gather_inplace(opt._flat_buf[lo:hi])
                    out[arm], out[arm + "_momentum"] = a.data.detach().clone(), opt._flat_buf.clone()
                out["consistent"] = check_replicas(a, world)
            elif mode == "shard16":
                out[arm], out[arm + "_momentum"] = master.clone(), mom.clone()
            else:
                out[arm] = a.data.detach().clone()
                m = torch.zeros_like(a.data)
                for i, p in enumerate(a.params):
                    a.shaped(m, i).copy_(opt.state[p]["momentum_buffer"])
                out[arm + "_momentum"] = m
        dist.destroy_process_group()
        q.put((rank, {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()}))
    except Exception:
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
        raise
