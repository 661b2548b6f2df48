#!/usr/bin/env python3
"""What LAMB (--optimizer lamb, optim/lamb.py) costs on the captured VGG-11 training step (one
MI355X), in-process, two arms on the same build:

    adamw        AdamW: one update launch
    lamb         LAMB: the norms launch in front of the update launch

    python tools/ab_lamb.py --batches 256,32
    python tools/ab_lamb.py --kernel      # the launches alone: AdamW's update, LAMB's norms + update,
                                          #   and LAMB's norms launch by itself with its bytes per second

lamb - adamw is the trust ratios' cost: one more dispatch per update launch, a norms pass that
streams p, g, m, v of the adapted tensors (16 B per element, nothing stored but one float2 per
8192-element chunk), and in the update launch a prologue that sums a tensor's partials. Both arms
keep every update in the step's own launch, so the known price of giving up SGD in the backward
(tools/ab_adamw.py) is in both. As tools/ab_adamw.py: arms alternate within each trial, a fresh
TrainStep is captured per arm and trial, ``--reps`` replays are timed with device events; one
JSON line per batch. ``--kernel`` times ``--reps`` launches back to back (device events, median
over ``--trials``).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
ARMS = ("adamw", "lamb")

from ab_adamw import _timed  # noqa: E402


def _median(v):
    return sorted(v)[len(v) // 2]


def kernel_times(a):
    import torch
    import ddp_amd
    from ddp_amd.models import build
    from ddp_amd.ops.common import native, stream_handle
    from ddp_amd.optim import AdamW, LAMB
    torch.manual_seed(ddp_amd.SEED)
    model = build("vgg11").cuda()
    opts = {"adamw": AdamW(model.parameters(), lr=0.0, weight_decay=0.0),
            "lamb": LAMB(model.parameters(), lr=0.0, weight_decay=0.0)}
    for sp in model.fused_plan():
        sp.maybe_pack()
    lamb = opts["lamb"]
    lamb.arena.grad.normal_()
    lamb.second_moment.fill_(1.0)
    arena = lamb.arena
    items, n_items = lamb._norm_table((0, len(arena.params)))
    adapted = sum(n for n, ad in zip(arena.numels, lamb._adapted()) if ad)

    def norms():
        native().lamb_norms(items.data_ptr(), n_items, arena.data.data_ptr(),
                            arena.grad.data_ptr(), lamb.momentum_buffer.data_ptr(), 0.0, 1.0,
                            lamb._trust_partial.data_ptr(), stream_handle(),
                            sched=lamb._sched_ptr(), **lamb._adam_kw())
    fns = {"adamw": lambda: opts["adamw"].step(lr_advance=False),
           "lamb": lambda: lamb.step(lr_advance=False), "lamb_norms": norms}
    res = {k: [] for k in fns}
    for _ in range(a.trials):
        for arm, fn in fns.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            res[arm].append(_timed(fn, a.reps) * 1e3)
    med = {k: _median(v) for k, v in res.items()}
    print(json.dumps({"launch_us": {k: round(v, 2) for k, v in med.items()},
                      "adapted_elements": adapted, "norm_blocks": n_items,
                      "norms_bytes_mb": round(adapted * 16 / 1e6, 1),
                      "norms_tb_per_s": round(adapted * 16 / (med["lamb_norms"] * 1e-6) / 1e12, 3),
                      "arena_mb": round(arena.total * 4 / 1e6, 1),
                      "all_us": {k: [round(x, 2) for x in v] for k, v in res.items()}}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,32")
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--kernel", action="store_true")
    a = ap.parse_args()
    if a.kernel:
        return kernel_times(a)
    import torch
    import ddp_amd
    from ddp_amd.data import DeviceLoader, SyntheticCIFAR10
    from ddp_amd.engine import CrossEntropyLoss, TrainStep
    from ddp_amd.models import build
    from ddp_amd.optim import AdamW, LAMB
    arms = a.arms.split(",")
    dev = torch.device("cuda", 0)
    for B in [int(b) for b in a.batches.split(",")]:
        torch.manual_seed(ddp_amd.SEED)
        loader = DeviceLoader(SyntheticCIFAR10(True), B, dev, 1, 0, train=True, cpad=8)
        model = build("vgg11").to(dev)
        opts = {"adamw": AdamW(model.parameters(), lr=1e-4),
                "lamb": LAMB(model.parameters(), lr=1e-4)}
        crit = CrossEntropyLoss()
        res = {v: [] for v in arms}
        for _ in range(a.trials):
            for v in arms:
                st = TrainStep(model, opts[v], crit, loader)
                assert st.opt_in_bwd is False
                st.warmup(2)
                st.capture()
                for _ in range(3):
                    st.step()
                torch.cuda.synchronize()
                res[v].append(_timed(st.step, a.reps))
                del st
            torch.cuda.empty_cache()
        print(json.dumps({"batch": B, "elements": sum(p.numel() for p in model.parameters()),
                          "median_ms": {v: round(_median(t), 4) for v, t in res.items()},
                          "all_ms": {v: [round(x, 4) for x in t] for v, t in res.items()}}),
              flush=True)
        del model, opts, loader
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
