"""Isolated times of the RepVGG block's normalisation passes (csrc/kernels/rep_bn.hip) on
RepVGG-A0's layer shapes, for CIFAR-size (32) and ImageNet-size (224) inputs.

Per shape: the library's forward (one launch, with the statistics of y) and backward (reduce +
apply), and next to them the composed path they replace, on the same session's kernels: three
bn_act_fwd passes (no ReLU) + two ATen adds + ReLU, and the ATen mask + three bn_act_bwd passes.
Three alternating passes; each figure is the median, the spread the range over the passes. Bytes
are the algorithmic ones (bf16) of the fused pass: forward nbr inputs + y, backward dy + y + nbr
inputs + nbr gradients.

    python tools/rep_bn_bench.py [--batch 256] [--inputs 32,224] [--widths 48,48,96,192,1280]
                                 [--out FILE.json]

bn_act_bwd's reduce needs a channel-group count that tiles 256 threads, so it refuses 48, 96, 192
and 1280 channels: the composed backward is then recorded as null (RepVGG-A1's 64, 128 and 256
are served: --widths 64,64,128,256,1280). The event times hold the launch gap.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.dwconv_bench import timed  # noqa: E402

# (stage, input size / output size, branches) of RepVGG-A's distinct blocks
LAYERS = ((0, 2, 2), (1, 4, 2), (1, 4, 3), (2, 8, 2), (2, 8, 3), (3, 16, 2), (3, 16, 3), (4, 32, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--inputs", default="32,224")
    ap.add_argument("--widths", default="48,48,96,192,1280", help="stage widths (default: A0)")
    ap.add_argument("--budget-s", type=float, default=0.1, help="timed window per figure")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ddp_amd
    from ddp_amd.ops.common import ptr, stat_replicas, stream_handle, workspace
    nat = ddp_amd.native()
    dev = torch.device("cuda", 0)
    torch.manual_seed(ddp_amd.SEED)
    N, nrep, rows = args.batch, stat_replicas(), []
    ws, st = workspace(dev), stream_handle()
    for size in (int(v) for v in args.inputs.split(",")):
        for stage, down, nbr in LAYERS:
            K, P = int(args.widths.split(",")[stage]), size // down
            bf = lambda: torch.randn(N, P, P, K, device=dev).to(torch.bfloat16)
            z, dz, t = [bf() for _ in range(nbr)], [bf() for _ in range(nbr)], [bf() for _ in range(nbr)]
            dy, y, g = bf(), bf(), bf()
            vec = lambda v: torch.full((K,), v, device=dev)
            gamma, beta, dg, db = vec(1.0), vec(0.0), vec(0.0), vec(0.0)
            stats, coef = [], [torch.empty(6 * K, device=dev) for _ in range(nbr)]
            for zi in z:
                s = torch.zeros(nrep, 2, K, device=dev)
                s[0, 0], s[0, 1] = zi.float().sum((0, 1, 2)), (zi.float() ** 2).sum((0, 1, 2))
                stats.append(s)
            ost, sums = torch.zeros(nrep, 2, K, device=dev), torch.zeros(nrep * 2 * K, device=dev)
            br = [(ptr(z[i]), ptr(stats[i]), ptr(gamma), ptr(beta), 0, 0, 0.1, 1e-5, ptr(coef[i]),
                   ptr(dz[i]), ptr(dg), ptr(db)) for i in range(nbr)]

            def composed_fwd():
                for i in range(nbr):
                    nat.bn_act_fwd(N, P, P, K, 0, 0, 1e-5, ptr(z[i]), 0, ptr(stats[i]), ptr(gamma),
                                   ptr(beta), ptr(t[i]), st, 0, 0, 0.1, 0, ptr(coef[i]))
                for i in range(1, nbr):
                    t[0].add_(t[i])
                torch.clamp_min(t[0], 0, out=y)  # the ReLU

            def composed_bwd():
                torch.mul(dy, y > 0, out=g)
                for i in range(nbr):
                    nat.bn_act_bwd(N, P, P, K, 0, 0, 1e-5, ptr(z[i]), 0, ptr(stats[i]), ptr(gamma),
                                   ptr(beta), ptr(g), ptr(sums), ptr(dz[i]), 0, ptr(dg), ptr(db), 0,
                                   st, ptr(coef[i]))

            fns = {
                "fwd": lambda: nat.rep_bn_fwd(N, P, P, K, br, ptr(y), ptr(ost), 0, st),
                "bwd": lambda: nat.rep_bn_bwd(N, P, P, K, br, ptr(dy), ptr(y), ptr(ws), ws.numel(), st),
                "composed_fwd": composed_fwd,
                "composed_bwd": composed_bwd,
            }
            try:
                composed_bwd()
            except RuntimeError:  # bn_act_bwd does not serve this channel count
                del fns["composed_bwd"]
            tm = {k: [] for k in fns}
            for _ in range(3):  # alternating passes
                for k, fn in fns.items():
                    tm[k].append(timed(fn, args.budget_s))
            med = {k: sorted(v)[1] for k, v in tm.items()}
            e = 2 * N * P * P * K  # bytes of one activation
            nb = {"fwd": (nbr + 1) * e, "bwd": (2 + 2 * nbr) * e}
            row = dict(N=N, P=P, K=K, branches=nbr,
                       us={k: round(v * 1e3, 2) for k, v in med.items()},
                       spread_us={k: round((max(v) - min(v)) * 1e3, 2) for k, v in tm.items()},
                       MB={k: round(v / 1e6, 2) for k, v in nb.items()},
                       GBps={k: round(nb[k] / med[k] / 1e6, 1) for k in nb},
                       fwd_vs_composed=round(med["fwd"] / med["composed_fwd"], 3),
                       bwd_vs_composed=(round(med["bwd"] / med["composed_bwd"], 3)
                                        if "composed_bwd" in med else None))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del z, dz, t, dy, y, g
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
