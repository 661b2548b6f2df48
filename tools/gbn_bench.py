"""Isolated times of the Ghost BatchNorm + ReLU (+ pool) kernels (csrc/kernels/ghost_bn.hip) on
the VGG-11 layer shapes (32x32 input).

Per shape and batch: the library's forward (stats + apply launches) and backward (reduce + apply
launches); PyTorch-ROCm's per-group composite, batch_norm on z[g::ngroups] -> relu -> max_pool2d
in bf16 channels_last (backward = autograd of it); and the library's BatchNorm streaming passes at
the same shape (bn_act_fwd = the apply pass, bn_act_bwd = reduce + finalize + apply; their
statistics come from the conv epilogue and are not in these figures). Three alternating passes;
each figure is the median, the spread is the range over the passes. The event times hold the
launch gaps (two launches each way for the ghost kernels).

    python tools/gbn_bench.py [--batches 256,32] [--ghost 32] [--layers 0,1,..] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.dwconv_bench import timed  # noqa: E402
from tools.gn_bench import LAYERS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,32")
    ap.add_argument("--ghost", type=int, default=32)
    ap.add_argument("--layers", default=None, help="indices into LAYERS (default: all)")
    ap.add_argument("--budget-s", type=float, default=0.25, help="timed window per figure")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ddp_amd
    from ddp_amd.ops.common import ptr, stat_replicas, stream_handle, workspace
    nat = ddp_amd.native()
    dev = torch.device("cuda", 0)
    torch.manual_seed(ddp_amd.SEED)
    G, rows = args.ghost, []
    for N in (int(v) for v in args.batches.split(",")):
        if N % G:
            ap.error("the torch composite here takes batches that are a multiple of --ghost")
        ng = N // G
        for C, H, pool in ([LAYERS[int(i)] for i in args.layers.split(",")] if args.layers
                           else LAYERS):
            Ho = H // 2 if pool else H
            z = torch.randn(N, H, H, C, device=dev).to(torch.bfloat16)
            dy = torch.randn(N, Ho, Ho, C, device=dev).to(torch.bfloat16)
            y, dz = torch.empty_like(dy), torch.empty_like(z)
            gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
            dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
            table = torch.empty(ng, 2, C, device=dev)
            nrep = stat_replicas()
            stats = torch.zeros(nrep * 2 * C, device=dev)
            stats[:C] = z.float().sum((0, 1, 2))
            stats[C:2 * C] = (z.float() ** 2).sum((0, 1, 2))
            sums = torch.zeros(nrep * 2 * C, device=dev)
            coef = torch.empty(6 * C, device=dev)
            ws, st = workspace(dev), stream_handle()
            zl = z.permute(0, 3, 1, 2).requires_grad_(True)  # NCHW view, channels_last memory
            gl, bl = gamma.bfloat16().requires_grad_(True), beta.bfloat16().requires_grad_(True)

            def torch_fwd():
                parts = [F.batch_norm(zl[g::ng], None, None, gl, bl, True, 0.0, 1e-5)
                         for g in range(ng)]
                a = F.relu(torch.stack(parts, 1).flatten(0, 1))  # image n = i * ng + g
                return F.max_pool2d(a, 2, 2) if pool else a

            yl, dyl = torch_fwd(), dy.permute(0, 3, 1, 2)
            head = (N, H, H, C, G, pool, 1, 1e-5, ptr(z), ptr(gamma), ptr(beta))
            fns = {
                "fwd": lambda: nat.gbn_act_fwd(*head, ptr(y), ptr(table), ptr(ws), ws.numel(), st),
                "bwd": lambda: nat.gbn_act_bwd(*head, ptr(table), ptr(dy), ptr(dz), ptr(dg),
                                               ptr(db), ptr(ws), ws.numel(), st),
                "torch_fwd": torch_fwd,
                "torch_bwd": lambda: torch.autograd.grad(yl, (zl, gl, bl), dyl, retain_graph=True),
                "bn_fwd": lambda: nat.bn_act_fwd(N, H, H, C, pool, 1, 1e-5, ptr(z), 0, ptr(stats),
                                                 ptr(gamma), ptr(beta), ptr(y), st, 0, 0, 0.1, 0,
                                                 ptr(coef)),
                "bn_bwd": lambda: nat.bn_act_bwd(N, H, H, C, pool, 1, 1e-5, ptr(z), 0, ptr(stats),
                                                 ptr(gamma), ptr(beta), ptr(dy), ptr(sums),
                                                 ptr(dz), 0, ptr(dg), ptr(db), 0, st, ptr(coef)),
            }
            fns["fwd"]()  # the backward reads the forward's table
            t = {k: [] for k in fns}
            for _ in range(3):  # alternating passes
                for k, fn in fns.items():
                    t[k].append(timed(fn, args.budget_s))
            med = {k: sorted(v)[1] for k, v in t.items()}
            row = dict(N=N, H=H, C=C, pool=pool, ghost=G,
                       us={k: round(v * 1e3, 2) for k, v in med.items()},
                       spread_us={k: round((max(v) - min(v)) * 1e3, 2) for k, v in t.items()},
                       fwd_vs_torch=round(med["fwd"] / med["torch_fwd"], 3),
                       bwd_vs_torch=round(med["bwd"] / med["torch_bwd"], 3),
                       fwd_vs_bn=round(med["fwd"] / med["bn_fwd"], 3),
                       bwd_vs_bn=round(med["bwd"] / med["bn_bwd"], 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del zl, yl
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
