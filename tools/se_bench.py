"""Isolated times of the Squeeze-and-Excitation tail (csrc/kernels/se.hip) on the bn3 shapes of
ResNet-50's four stages (224x224 input).

Per shape and batch: se_fwd (finalize, squeeze, excite, apply) and se_bwd (reduce, excite_bwd,
param_bwd, apply_bwd) of the library; the library's plain residual BatchNorm passes at the same
shape (bn_act_fwd / bn_act_bwd with a residual and the ReLU mask); and PyTorch-ROCm's composite
under bf16 autocast on the BatchNorm output (adaptive_avg_pool2d, two linears, multiply, add,
relu; backward = autograd of those). Three alternating passes; each figure is the median, the
spread is the range over the passes.

    python tools/se_bench.py [--batches 256,32] [--stages 0,1,2,3] [--out FILE.json]

The event times hold the launch gaps (four launches each way). For kernel-only times run one shape
per process under a kernel trace (``--stages I --batches N --budget-s 0.02``).
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.dwconv_bench import timed  # noqa: E402

STAGES = ((256, 56), (512, 28), (1024, 14), (2048, 7))  # (channels, bn3 output size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,32")
    ap.add_argument("--stages", default="0,1,2,3")
    ap.add_argument("--reduction", type=int, default=16)
    ap.add_argument("--budget-s", type=float, default=0.25, help="timed window per figure")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ddp_amd
    from ddp_amd.ops.common import ptr, stat_replicas, stream_handle, workspace
    nat = ddp_amd.native()
    dev = torch.device("cuda", 0)
    torch.manual_seed(ddp_amd.SEED)
    red, rows = args.reduction, []
    for N in (int(v) for v in args.batches.split(",")):
        for C, H in (STAGES[int(i)] for i in args.stages.split(",")):
            Cr = C // red
            bf = lambda: torch.randn(N, H, H, C, device=dev).to(torch.bfloat16)
            f32 = lambda *s: torch.empty(*s, device=dev)
            z, res, dy = bf(), bf(), bf()
            y, dz, dres = (torch.empty_like(z) for _ in range(3))
            mask = torch.empty(N, H, H, C // 8, dtype=torch.uint8, device=dev)
            gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
            fc1, fc2 = torch.nn.Linear(C, Cr).to(dev), torch.nn.Linear(Cr, C).to(dev)
            nrep = stat_replicas()
            stats = torch.zeros(nrep * 2 * C, device=dev)
            stats[:C] = z.float().sum((0, 1, 2))
            stats[C:2 * C] = (z.float() ** 2).sum((0, 1, 2))
            sums, coef = torch.zeros(nrep * 2 * C, device=dev), f32(6 * C)
            S, s, h, G = f32(N, C), f32(N, C), f32(N, Cr), f32(2, N, C)
            dt2, dh, dm = f32(N, C), f32(N, Cr), f32(N, C)
            gr = [torch.zeros_like(p) for p in (fc1.weight, fc1.bias, fc2.weight, fc2.bias,
                                                gamma, beta)]
            ws, st = workspace(dev), stream_handle()
            ul = (z.float() * 0.5).to(torch.bfloat16).permute(0, 3, 1, 2).requires_grad_(True)
            rl = res.permute(0, 3, 1, 2)

            def torch_fwd():
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    g = torch.sigmoid(fc2(F.relu(fc1(F.adaptive_avg_pool2d(ul, 1).flatten(1)))))
                    return F.relu(ul * g[:, :, None, None] + rl)

            yl, dyl = torch_fwd(), dy.permute(0, 3, 1, 2)
            tp = (ul, fc1.weight, fc1.bias, fc2.weight, fc2.bias)
            fns = {
                "fwd": lambda: nat.se_fwd(N, H, H, C, red, 1e-5, ptr(z), ptr(res), ptr(stats),
                                          ptr(gamma), ptr(beta), ptr(coef), ptr(fc1.weight),
                                          ptr(fc1.bias), ptr(fc2.weight), ptr(fc2.bias), ptr(S),
                                          ptr(s), ptr(h), ptr(y), ptr(mask), ptr(ws), ws.numel(),
                                          st),
                "bwd": lambda: nat.se_bwd(N, H, H, C, red, ptr(z), ptr(dy), ptr(mask), ptr(coef),
                                          ptr(fc1.weight), ptr(fc2.weight), ptr(S), ptr(s), ptr(h),
                                          ptr(G), ptr(dt2), ptr(dh), ptr(dm), *(ptr(g) for g in gr),
                                          ptr(dz), ptr(dres), ptr(ws), ws.numel(), st),
                "torch_fwd": torch_fwd,
                "torch_bwd": lambda: torch.autograd.grad(yl, tp, dyl, retain_graph=True),
                "bn_fwd": lambda: nat.bn_act_fwd(N, H, H, C, 0, 1, 1e-5, ptr(z), ptr(res),
                                                 ptr(stats), ptr(gamma), ptr(beta), ptr(y), st, 0,
                                                 0, 0.1, 0, ptr(coef), mask=ptr(mask)),
                "bn_bwd": lambda: nat.bn_act_bwd(N, H, H, C, 0, 1, 1e-5, ptr(z), 0, ptr(stats),
                                                 ptr(gamma), ptr(beta), ptr(dy), ptr(sums),
                                                 ptr(dz), ptr(dres), ptr(gr[4]), ptr(gr[5]), 0, st,
                                                 ptr(coef), mask=ptr(mask)),
            }
            t = {k: [] for k in fns}
            for _ in range(3):  # alternating passes
                for k, fn in fns.items():
                    if k == "bwd":
                        fns["fwd"]()  # the backward reads the forward's tables and mask
                    if k == "bn_bwd":
                        fns["bn_fwd"]()
                        sums.zero_()
                    t[k].append(timed(fn, args.budget_s))
            med = {k: sorted(v)[1] for k, v in t.items()}
            row = dict(N=N, H=H, C=C, Cr=Cr,
                       us={k: round(v * 1e3, 2) for k, v in med.items()},
                       spread_us={k: round((max(v) - min(v)) * 1e3, 2) for k, v in t.items()},
                       fwd_vs_bn=round(med["fwd"] / med["bn_fwd"], 3),
                       bwd_vs_bn=round(med["bwd"] / med["bn_bwd"], 3),
                       fwd_vs_torch=round(med["fwd"] / med["torch_fwd"], 3),
                       bwd_vs_torch=round(med["bwd"] / med["torch_bwd"], 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del ul, yl
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
