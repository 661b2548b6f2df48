#!/usr/bin/env python3
"""Where a conv GEMM work item spends its cycles: setup, k-loop, epilogue (one MI355X).

    python tools/probes/conv_item_stamps.py [--batches 256 32] [--md out.md] [--json out.json]

Runs each of VGG-11's eight conv layers once per batch — forward, then the backward pair (or
the lone WGRAD of the input layer) — through the "stamps" diagnostic build of the extension
(_build.py variant "stamps", -DDDP_CONV_STAMPS: csrc/kernels/common.h ConvStampBuf). Every work
item of conv_igemm_kernel, conv_bwd_pair_kernel and conv_tr_fwd_kernel records the shader-clock
cycles its first wave spent in

  setup     index math and gather state before the first operand load,
  k-loop    prologue DMA + the MFMA loop,
  epilogue  stores, statistics, split-K slab writes,

and the tool prints the three shares per layer and phase (median item, and the sum over items).
The ops are launched as tools/conv_bench.py launches them: the training step's tile, split and
kernel selection, without the step's cross-layer fusions (fused BN input, BN-backward sums, SGD
in the WGRAD epilogue). Layer 1 of the training step runs in conv_l0.hip, which is not stamped.

The stamps build is made on first use (several minutes of hipcc) unless DDP_AMD_NATIVE_PATH
already names one. The shipped builds contain no stamp code.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

PHASES = {0: "FWD", 1: "DGRAD", 2: "WGRAD", 3: "FWD tap-reuse"}
CAP = 1 << 16  # records per launch (VGG-11 b256: at most ~10k items)


def vgg_layers(B):
    cfg = [(3, 64, 32), (64, 128, 16), (128, 256, 8), (256, 256, 8), (256, 512, 4),
           (512, 512, 4), (512, 512, 2), (512, 512, 2)]
    return [(B, 8 if cin == 3 else cin, h, h, k, 3, 1, 1, cin) for cin, k, h in cfg]


def summarise(rec):
    """rec: int tensor [n][4] = tag, setup, k-loop, epilogue -> {phase: row}"""
    out = {}
    for tag, name in PHASES.items():
        r = rec[rec[:, 0] == tag]
        if r.shape[0] == 0:
            continue
        tot = r[:, 1:].sum(dim=0).tolist()
        life = float(sum(tot)) or 1.0
        med = [statistics.median(r[:, c].tolist()) for c in (1, 2, 3)]
        out[name] = {"items": int(r.shape[0]),
                     "median_cycles": [int(m) for m in med],
                     "share_pct": [round(100.0 * t / life, 1) for t in tot]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 32])
    ap.add_argument("--md", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not os.environ.get("DDP_AMD_NATIVE_PATH"):
        from importlib import import_module
        b = import_module("ddp_amd._build")
        b.build(verbose=True, variants=("stamps",))
        os.environ["DDP_AMD_NATIVE_PATH"] = b.ext_path("stamps")
    import torch
    import ddp_amd
    from ddp_amd.ops.layers import ConvBNActSpec, conv_forward, conv_backward
    nat = ddp_amd.native()
    if not hasattr(nat, "conv_stamps_set"):
        raise SystemExit("the loaded extension is not a stamps build (-DDDP_CONV_STAMPS)")
    dev = torch.device("cuda", 0)
    buf = torch.zeros(4 + 4 * CAP, dtype=torch.int32, device=dev)

    def stamped(fn):
        fn()  # unstamped first run: weight packing, function attributes, caches
        torch.cuda.synchronize()
        buf.zero_()
        nat.conv_stamps_set(buf.data_ptr(), CAP)
        fn()
        torch.cuda.synchronize()
        nat.conv_stamps_set(0, 0)
        n = min(int(buf[0]), CAP)
        return buf[4:4 + 4 * n].view(n, 4).cpu()

    rows = []
    for B in args.batches:
        for li, (N, C, H, W, K, R, stride, pad, Cr) in enumerate(vgg_layers(B)):
            conv = torch.nn.Conv2d(Cr, K, R, stride, pad, bias=False).to(dev)
            conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)
            spec = ConvBNActSpec(conv, None, cin_pad=C if C != Cr else None)
            spec.maybe_pack()
            x = torch.randn(N, H, W, C, device=dev).to(torch.bfloat16)
            dz = torch.randn(N, H, W, K, device=dev).to(torch.bfloat16)
            dw = torch.zeros_like(conv.weight)
            stats = torch.zeros(16 * 2 * K, device=dev)
            ops = {"fwd": lambda: conv_forward(spec, x, None, stats),
                   "bwd": lambda: conv_backward(spec, x, dz, dw, C == Cr)}
            for op, fn in ops.items():
                for phase, s in summarise(stamped(fn)).items():
                    rows.append({"batch": B, "layer": li + 1, "shape": f"{Cr}->{K} {H}x{W}",
                                 "op": op, "phase": phase, **s})
    lines = ["| batch | layer | shape | phase | items | median cycles setup / k-loop / epilogue "
             "| share % setup / k-loop / epilogue | setup + epilogue % |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        m, s = r["median_cycles"], r["share_pct"]
        lines.append(f"| {r['batch']} | {r['layer']} | {r['shape']} | {r['phase']} | {r['items']} | "
                     f"{m[0]} / {m[1]} / {m[2]} | {s[0]} / {s[1]} / {s[2]} | {round(s[0] + s[2], 1)} |")
    text = "\n".join(lines)
    print(text)
    if args.md:
        with open(args.md, "w") as f:
            f.write(text + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
