"""Isolated times of the depthwise 3x3 kernels (csrc/kernels/dwconv.hip) on MobileNet v1's layers.

Per shape: forward, DGRAD and WGRAD (+ finish) of the library, PyTorch-ROCm's
F.conv2d(groups=C) in bf16 channels_last (forward; backward = input and weight gradient), and
the library's bn_act_fwd streaming pass over a tensor of the output's size. Three alternating
passes; each figure is the median, the spread is the range over the passes. Bytes are counted
from the shapes (bf16): fwd in + out, dgrad dz + dx, wgrad dz + x.

    python tools/dwconv_bench.py [--batch 256] [--inputs 224,32] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (channels, stride, input size / layer size) of the depthwise layers; the five 512-channel
# stride-1 layers share a shape (1024 x 7 x 7 at stride 2 -> 1 is the 512 s2 layer's neighbour)
LAYERS = ((32, 1, 2), (64, 2, 2), (128, 1, 4), (128, 2, 4), (256, 1, 8), (256, 2, 8), (512, 1, 16),
          (512, 2, 16), (1024, 1, 32))


def timed(fn, budget_s=0.25):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    reps = max(5, min(2000, int(budget_s * 1e3 / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps  # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--inputs", default="224,32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ddp_amd
    from ddp_amd.ops.common import ptr, stat_replicas, stream_handle, workspace
    nat = ddp_amd.native()
    dev = torch.device("cuda", 0)
    torch.manual_seed(ddp_amd.SEED)
    rows = []
    for size in (int(v) for v in args.inputs.split(",")):
        for C, s, div in LAYERS:
            N, H = args.batch, size // div
            P = (H - 1) // s + 1
            x = torch.randn(N, H, H, C, device=dev).to(torch.bfloat16)
            dz = torch.randn(N, P, P, C, device=dev).to(torch.bfloat16)
            wc = torch.randn(C, 3, 3, 8, device=dev).to(torch.bfloat16)
            z, dx = torch.empty_like(dz), torch.empty_like(x)
            dw = torch.zeros(C, 1, 3, 3, device=dev)
            nrep = stat_replicas()
            stats = torch.zeros(nrep * 2 * C, device=dev)
            gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
            coef, y = torch.empty(6 * C, device=dev), torch.empty_like(z)
            ws = workspace(dev)
            g = (N, H, H, C, C, 3, 3, s, 1, P, P, 1, 0)
            st = stream_handle()
            xl = x.permute(0, 3, 1, 2).requires_grad_(True)  # NCHW view, channels_last memory
            wl = wc[..., 0].unsqueeze(1).contiguous().requires_grad_(True)
            dzl = dz.permute(0, 3, 1, 2)
            zl = F.conv2d(xl, wl, None, s, 1, groups=C)
            fns = {
                "fwd": lambda: nat.dwconv_fwd(g, C, ptr(x), ptr(wc), 0, ptr(z), ptr(stats), st),
                "dgrad": lambda: nat.dwconv_dgrad(g, C, ptr(dz), ptr(wc), ptr(dx), st),
                "wgrad": lambda: nat.dwconv_wgrad(g, C, ptr(dz), ptr(x), ptr(dw), ptr(ws),
                                                  ws.numel(), st),
                "lib_fwd": lambda: F.conv2d(xl, wl, None, s, 1, groups=C),
                "lib_bwd": lambda: torch.autograd.grad(zl, (xl, wl), dzl, retain_graph=True),
                "stream": lambda: nat.bn_act_fwd(N, P, P, C, 0, 1, 1e-5, ptr(z), 0, ptr(stats),
                                                 ptr(gamma), ptr(beta), ptr(y), st, 0, 0, 0.1, 0,
                                                 ptr(coef)),
            }
            t = {k: [] for k in fns}
            for _ in range(3):  # alternating passes
                for k, fn in fns.items():
                    t[k].append(timed(fn))
            med = {k: sorted(v)[1] for k, v in t.items()}
            spread = {k: max(v) - min(v) for k, v in t.items()}
            nb = {"fwd": 2 * (x.numel() + z.numel()), "dgrad": 2 * (x.numel() + z.numel()),
                  "wgrad": 2 * (x.numel() + z.numel()), "stream": 4 * z.numel()}
            bwd = med["dgrad"] + med["wgrad"]
            row = dict(input=size, N=N, H=H, C=C, stride=s,
                       ms={k: round(v, 4) for k, v in med.items()},
                       spread_ms={k: round(v, 4) for k, v in spread.items()},
                       GBps={k: round(nb[k] / med[k] / 1e6, 1) for k in nb},
                       fwd_vs_lib=round(med["fwd"] / med["lib_fwd"], 3),
                       bwd_vs_lib=round(bwd / med["lib_bwd"], 3),
                       fwd_ok=med["fwd"] <= med["lib_fwd"] + spread["lib_fwd"],
                       bwd_ok=bwd <= med["lib_bwd"] + spread["lib_bwd"],
                       fwd_vs_stream=round(med["fwd"] / med["stream"], 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del xl, wl, zl
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
