"""Isolated times of the GroupNorm + ReLU (+ pool) kernels (csrc/kernels/group_norm.hip) on the
VGG-11 layer shapes (32x32 input).

Per shape and batch: forward and backward (+ finish) of the library; PyTorch-ROCm's
group_norm -> relu -> max_pool2d in bf16 channels_last (forward; backward = autograd of the
three); and the library's BatchNorm streaming passes at the same shape (bn_act_fwd = the apply
pass, bn_act_bwd = reduce + finalize + apply). Three alternating passes; each figure is the
median, the spread is the range over the passes. Bytes are the algorithmic ones (bf16): forward
z + y, backward z + dy + dz.

    python tools/gn_bench.py [--batches 256,32] [--groups 32] [--layers 0,1,..] [--out FILE.json]

The event times hold the launch gap. For kernel-only times run one shape per process under a
kernel trace (``--layers I --batches N --budget-s 0.02``) and read the per-kernel statistics.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.dwconv_bench import timed  # noqa: E402

# (channels, conv output size, pooled) of VGG-11's eight blocks
LAYERS = ((64, 32, 1), (128, 16, 1), (256, 8, 0), (256, 8, 1), (512, 4, 0), (512, 4, 1),
          (512, 2, 0), (512, 2, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,32")
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--layers", default=None, help="indices into LAYERS (default: all)")
    ap.add_argument("--budget-s", type=float, default=0.25, help="timed window per figure")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ddp_amd
    from ddp_amd.ops.common import ptr, stat_replicas, stream_handle, workspace
    nat = ddp_amd.native()
    dev = torch.device("cuda", 0)
    torch.manual_seed(ddp_amd.SEED)
    G, rows = args.groups, []
    for N in (int(v) for v in args.batches.split(",")):
        for C, H, pool in ([LAYERS[int(i)] for i in args.layers.split(",")] if args.layers
                           else LAYERS):
            Ho = H // 2 if pool else H
            z = torch.randn(N, H, H, C, device=dev).to(torch.bfloat16)
            dy = torch.randn(N, Ho, Ho, C, device=dev).to(torch.bfloat16)
            y, dz = torch.empty_like(dy), torch.empty_like(z)
            gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
            dg, db, dbias = (torch.zeros(C, device=dev) for _ in range(3))
            table = torch.empty(N, G, 2, device=dev)
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
                a = F.relu(F.group_norm(zl, G, gl, bl, 1e-5))
                return F.max_pool2d(a, 2, 2) if pool else a

            yl, dyl = torch_fwd(), dy.permute(0, 3, 1, 2)
            fns = {
                "fwd": lambda: nat.gn_act_fwd(N, H, H, C, G, pool, 1, 1e-5, ptr(z), ptr(gamma),
                                              ptr(beta), ptr(y), ptr(table), st),
                "bwd": lambda: nat.gn_act_bwd(N, H, H, C, G, pool, 1, 1e-5, ptr(z), ptr(gamma),
                                              ptr(beta), ptr(table), ptr(dy), ptr(dz), ptr(dg),
                                              ptr(db), ptr(dbias), ptr(ws), ws.numel(), st),
                "torch_fwd": torch_fwd,
                "torch_bwd": lambda: torch.autograd.grad(yl, (zl, gl, bl), dyl, retain_graph=True),
                "bn_fwd": lambda: nat.bn_act_fwd(N, H, H, C, pool, 1, 1e-5, ptr(z), 0, ptr(stats),
                                                 ptr(gamma), ptr(beta), ptr(y), st, 0, 0, 0.1, 0,
                                                 ptr(coef)),
                "bn_bwd": lambda: nat.bn_act_bwd(N, H, H, C, pool, 1, 1e-5, ptr(z), 0, ptr(stats),
                                                 ptr(gamma), ptr(beta), ptr(dy), ptr(sums),
                                                 ptr(dz), 0, ptr(dg), ptr(db), ptr(dbias), st,
                                                 ptr(coef)),
            }
            fns["fwd"]()  # the backward reads the forward's table
            t = {k: [] for k in fns}
            for _ in range(3):  # alternating passes
                for k, fn in fns.items():
                    t[k].append(timed(fn, args.budget_s))
            med = {k: sorted(v)[1] for k, v in t.items()}
            spread = {k: max(v) - min(v) for k, v in t.items()}
            fb, bb = 2 * (z.numel() + y.numel()), 2 * (2 * z.numel() + y.numel())
            nb = {"fwd": fb, "bwd": bb, "torch_fwd": fb, "torch_bwd": bb, "bn_fwd": fb, "bn_bwd": bb}
            row = dict(N=N, H=H, C=C, pool=pool, groups=G,
                       us={k: round(v * 1e3, 2) for k, v in med.items()},
                       spread_us={k: round(v * 1e3, 2) for k, v in spread.items()},
                       GBps={k: round(nb[k] / med[k] / 1e6, 1) for k in nb},
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
