#!/usr/bin/env python3
"""What AdamW (--optimizer adamw, optim/adamw.py) costs on the captured VGG-11 training step
(one MI355X), in-process, three arms on the same build:

    sgd_bwd      FusedSGD, SGD in the backward (the default step)
    sgd_nobwd    FusedSGD with DDP_AMD_SGD_IN_BWD=0: every update in the step's own launch
    adamw        AdamW (its updates always run in the step's own launch)

    python tools/ab_adamw.py --batches 256,32
    python tools/ab_adamw.py --kernel      # the update launch alone, SGD and AdamW

adamw - sgd_nobwd is the rule's own cost: one more fp32 arena read and written inside the update
launch (about 34 B per element against 26 B) and a square root and a division per element, no
dispatch. sgd_nobwd - sgd_bwd is the known price of giving up SGD in the backward, which AdamW
shares with LARS, the guard, accumulation and the EMA. As tools/ab_ema.py: arms alternate within
each trial, a fresh TrainStep is captured per arm and trial, ``--reps`` replays are timed with
device events; one JSON line per batch. ``--kernel`` times ``--reps`` whole-arena update launches
of the VGG-11 optimizers back to back (device events, median over ``--trials``).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ARMS = ("sgd_bwd", "sgd_nobwd", "adamw")


def _timed(fn, reps):
    import torch
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_times(a):
    import torch
    import ddp_amd
    from ddp_amd.models import build
    from ddp_amd.optim import AdamW, FusedSGD
    torch.manual_seed(ddp_amd.SEED)
    model = build("vgg11").cuda()
    opts = {"sgd": FusedSGD(model.parameters(), lr=0.0, momentum=0.9, weight_decay=0.0),
            "adamw": AdamW(model.parameters(), lr=0.0, weight_decay=0.0)}
    opt = opts["sgd"]
    for sp in model.fused_plan():
        sp.maybe_pack()
    res = {"sgd": [], "adamw": []}
    for _ in range(a.trials):
        for arm in ("sgd", "adamw"):
            for _ in range(3):
                opts[arm].step(lr_advance=False)
            torch.cuda.synchronize()
            res[arm].append(_timed(lambda: opts[arm].step(lr_advance=False), a.reps) * 1e3)
    print(json.dumps({"update_launch_us": {k: round(sorted(v)[len(v) // 2], 2)
                                           for k, v in res.items()},
                      "arena_mb": round(opt.arena.total * 4 / 1e6, 1),
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
    from ddp_amd.optim import AdamW, FusedSGD
    arms = a.arms.split(",")
    dev = torch.device("cuda", 0)
    for B in [int(b) for b in a.batches.split(",")]:
        torch.manual_seed(ddp_amd.SEED)
        loader = DeviceLoader(SyntheticCIFAR10(True), B, dev, 1, 0, train=True, cpad=8)
        model = build("vgg11").to(dev)
        hp = dict(lr=0.01, momentum=0.9, weight_decay=1e-4)
        opts = {v: FusedSGD(model.parameters(), **hp) for v in ARMS[:2]}
        opts["adamw"] = AdamW(model.parameters(), lr=1e-4)
        crit = CrossEntropyLoss()
        res = {v: [] for v in arms}
        for _ in range(a.trials):
            for v in arms:
                os.environ["DDP_AMD_SGD_IN_BWD"] = "1" if v == "sgd_bwd" else "0"
                st = TrainStep(model, opts[v], crit, loader)
                assert st.opt_in_bwd is (v == "sgd_bwd")
                st.warmup(2)
                st.capture()
                for _ in range(3):
                    st.step()
                torch.cuda.synchronize()
                res[v].append(_timed(st.step, a.reps))
                del st
            torch.cuda.empty_cache()
        med = {v: sorted(t)[len(t) // 2] for v, t in res.items()}
        print(json.dumps({"batch": B, "elements": sum(p.numel() for p in model.parameters()),
                          "median_ms": {v: round(m, 4) for v, m in med.items()},
                          "all_ms": {v: [round(x, 4) for x in t] for v, t in res.items()}}),
              flush=True)
        del model, opts, loader
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
