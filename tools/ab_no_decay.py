#!/usr/bin/env python3
"""What the no-decay mask (--no-decay-1d, optim/sgd.py ``no_decay``) costs on the captured VGG-11
training step (one MI355X), in-process, two arms on the same build:

    sgd          FusedSGD, SGD in the backward (the default step)
    sgd_mask     FusedSGD(no_decay="1d"): the same step, bit 8 set in the kind word of the work
                 items of biases and BatchNorm vectors

    python tools/ab_no_decay.py --batches 256,32
    python tools/ab_no_decay.py --kernel      # the whole-arena update launch alone, four optimizers
    python tools/ab_no_decay.py --dispatches  # kernel dispatches of one replay, both arms

The mask adds no launch, no kernel argument and no table row, and the bytes streamed are the
same: the expectation is no difference. As tools/ab_adamw.py: arms alternate within each trial, a
fresh TrainStep is captured per arm and trial, ``--reps`` replays are timed with device events;
one JSON line per batch. ``--kernel`` times ``--reps`` whole-arena update launches back to back
(device events, median over ``--trials``), masked and unmasked, for SGD, LARS, AdamW and LAMB.
``--dispatches`` counts the kernel dispatches of one replay of each arm's captured step (the
profiler's device records) and must print equal numbers.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ARMS = ("sgd", "sgd_mask")


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
    from ddp_amd.optim import LAMB, LARS, AdamW, FusedSGD
    torch.manual_seed(ddp_amd.SEED)
    model = build("vgg11").cuda()
    mk = {"sgd": lambda m: FusedSGD(model.parameters(), lr=0.0, momentum=0.9, weight_decay=1e-4,
                                    no_decay=m),
          "lars": lambda m: LARS(model.parameters(), lr=0.0, momentum=0.9, weight_decay=1e-4,
                                 no_decay=m),
          "adamw": lambda m: AdamW(model.parameters(), lr=0.0, no_decay=m),
          "lamb": lambda m: LAMB(model.parameters(), lr=0.0, no_decay=m)}
    opts = {f"{k}{'_mask' if m else ''}": f(m) for k, f in mk.items() for m in (None, "1d")}
    for sp in model.fused_plan():
        sp.maybe_pack()
    res = {k: [] for k in opts}
    for _ in range(a.trials):
        for arm, opt in opts.items():
            for _ in range(3):
                opt.step(lr_advance=False)
            torch.cuda.synchronize()
            res[arm].append(_timed(lambda: opt.step(lr_advance=False), a.reps) * 1e3)
    print(json.dumps({"update_launch_us": {k: round(sorted(v)[len(v) // 2], 2)
                                           for k, v in res.items()},
                      "masked_items": int((opts["sgd_mask"]._work_table()[0][:, 0] & 0x100).ne(0).sum()),
                      "items": int(opts["sgd_mask"]._work_table()[1]),
                      "all_us": {k: [round(x, 2) for x in v] for k, v in res.items()}}),
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
    from ddp_amd.data import DeviceLoader, SyntheticCIFAR10
    from ddp_amd.engine import CrossEntropyLoss, TrainStep
    from ddp_amd.models import build
    from ddp_amd.optim import FusedSGD
    dev = torch.device("cuda", 0)
    for B in [int(b) for b in a.batches.split(",")]:
        torch.manual_seed(ddp_amd.SEED)
        loader = DeviceLoader(SyntheticCIFAR10(True), B, dev, 1, 0, train=True, cpad=8)
        model = build("vgg11").to(dev)
        hp = dict(lr=0.01, momentum=0.9, weight_decay=1e-4)
        opts = {"sgd": FusedSGD(model.parameters(), **hp),
                "sgd_mask": FusedSGD(model.parameters(), no_decay="1d", **hp)}
        crit = CrossEntropyLoss()
        res = {v: [] for v in ARMS}
        nodes = {}
        for _ in range(1 if a.dispatches else a.trials):
            for v in ARMS:
                st = TrainStep(model, opts[v], crit, loader)
                assert st.opt_in_bwd is True
                st.warmup(2)
                st.capture()
                for _ in range(3):
                    st.step()
                torch.cuda.synchronize()
                if a.dispatches:
                    nodes[v] = _dispatches(st)
                else:
                    res[v].append(_timed(st.step, a.reps))
                del st
            torch.cuda.empty_cache()
        if a.dispatches:
            print(json.dumps({"batch": B, "dispatches": nodes}), flush=True)
        else:
            med = {v: sorted(t)[len(t) // 2] for v, t in res.items()}
            print(json.dumps({"batch": B, "median_ms": {v: round(m, 4) for v, m in med.items()},
                              "all_ms": {v: [round(x, 4) for x in t] for v, t in res.items()}}),
                  flush=True)
        del model, opts, loader
        torch.cuda.empty_cache()


def _dispatches(st):
    """Kernel dispatches of one replay of the captured step, from the profiler's device activity
    records (copies and fills are no dispatches), as tests/ema_probe.py counts them."""
    import re
    import torch
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        st.step()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA
             and not re.match(r"(?i)(memcpy|memset|hipmemcpy|hipmemset|copy|fill)", e.name)]
    return len(names)


if __name__ == "__main__":
    main()
