#!/usr/bin/env python3
"""The wide classifier head (csrc/kernels/linear_wide.hip, --num-classes 17..128) on one MI355X.

    python tools/ab_wide_head.py --kernel       # the two launches alone against PyTorch-ROCm
    python tools/ab_wide_head.py                # the captured VGG-11 step, 10 against 100 classes
    python tools/ab_wide_head.py --dispatches   # kernel dispatches of one replay of each

``--kernel``: forward (logits-free: loss + dlogits) and backward (dx, dW, db) at F = 512,
J = 100, B = 32 and 256, each timed as ``--reps`` replays of a captured graph of 20 launches
(device events, median over ``--trials``), next to bf16 ``matmul`` + ``F.cross_entropy`` and
their autograd backward captured the same way. A yardstick, not a gate. The step arms alternate
within each trial, a fresh TrainStep is captured per arm and trial (as tools/ab_no_decay.py).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools.ab_no_decay import _dispatches, _timed  # noqa: E402

INNER = 20  # launches per captured graph of the kernel timings


def _graph(fn):
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(INNER):
            fn()
    return g


def kernel_times(a):
    import torch
    import torch.nn.functional as F
    from ddp_amd.ops.common import native, ptr, stream_handle
    nat, Fi, J = native(), 512, 100
    for B in (32, 256):
        x = torch.randn(B, Fi, device="cuda").to(torch.bfloat16)
        W = (torch.randn(J, Fi, device="cuda") * 0.05).requires_grad_(True)
        b = torch.zeros(J, device="cuda", requires_grad=True)
        y = torch.randint(0, J, (B,), device="cuda")
        dl, loss = torch.empty(B, J, device="cuda"), torch.zeros((), device="cuda")
        dx, dW, db = torch.empty_like(x), torch.zeros_like(W), torch.zeros_like(b)
        g1 = torch.ones(1, device="cuda")
        xr = x.clone().requires_grad_(True)

        def hip_fwd():
            nat.linear_ce_fwd(ptr(x), ptr(W), ptr(b), ptr(y), B, Fi, J, 0, ptr(dl), ptr(loss), 0,
                              stream_handle())

        def hip_bwd():
            nat.linear_bwd(ptr(dl), ptr(x), ptr(W), B, Fi, J, ptr(g1), ptr(dx), ptr(dW), ptr(db),
                           stream_handle())

        def torch_fwd():
            return F.cross_entropy((xr @ W.to(torch.bfloat16).t()).float() + b, y)

        def torch_fwd_bwd():
            xr.grad = W.grad = b.grad = None
            torch_fwd().backward()
        arms = {"hip_fwd": hip_fwd, "hip_bwd": hip_bwd, "torch_fwd": torch_fwd,
                "torch_fwd_bwd": torch_fwd_bwd}
        graphs = {k: _graph(f) for k, f in arms.items()}
        res = {k: [] for k in arms}
        for _ in range(a.trials):
            for k, g in graphs.items():
                res[k].append(_timed(g.replay, a.reps) / INNER * 1e3)
        print(json.dumps({"B": B, "F": Fi, "J": J,
                          "median_us": {k: round(sorted(v)[len(v) // 2], 2) for k, v in res.items()},
                          "all_us": {k: [round(t, 2) for t in v] for k, v in res.items()}}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,32")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--dispatches", action="store_true")
    a = ap.parse_args()
    if a.kernel:
        return kernel_times(a)
    import torch
    import ddp_amd
    from ddp_amd.data import DeviceLoader, SyntheticCIFAR10, SyntheticCIFAR100
    from ddp_amd.engine import CrossEntropyLoss, TrainStep
    from ddp_amd.models import build
    from ddp_amd.optim import FusedSGD
    dev = torch.device("cuda", 0)
    for B in [int(b) for b in a.batches.split(",")]:
        torch.manual_seed(ddp_amd.SEED)
        arms = {}
        for nc, ds in ((10, SyntheticCIFAR10(True)), (100, SyntheticCIFAR100(True))):
            model = build("vgg11", nc).to(dev)
            arms[nc] = (model, FusedSGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4),
                        DeviceLoader(ds, B, dev, 1, 0, train=True, cpad=8))
        res, nodes = {nc: [] for nc in arms}, {}
        for _ in range(1 if a.dispatches else a.trials):
            for nc, (model, opt, loader) in arms.items():
                st = TrainStep(model, opt, CrossEntropyLoss(), loader)
                st.warmup(2)
                st.capture()
                for _ in range(3):
                    st.step()
                torch.cuda.synchronize()
                if a.dispatches:
                    _dispatches(st)  # (the process's first profile can miss records)
                    nodes[nc] = _dispatches(st)
                else:
                    res[nc].append(_timed(st.step, a.reps))
                del st
        if a.dispatches:
            print(json.dumps({"batch": B, "dispatches": nodes}), flush=True)
        else:
            print(json.dumps({"batch": B,
                              "median_ms": {nc: round(sorted(t)[len(t) // 2], 4) for nc, t in res.items()},
                              "all_ms": {nc: [round(x, 4) for x in t] for nc, t in res.items()}}),
                  flush=True)
        del arms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
