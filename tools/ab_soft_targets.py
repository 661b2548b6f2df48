#!/usr/bin/env python3
"""What label smoothing and mixup cost on the captured VGG-11 training step (one MI355X),
in-process, four arms on the same build:

    plain     CrossEntropyLoss(), no mixup (the step as it was)
    smooth    label_smoothing 0.1 (the SOFT head kernel)
    mixup     mixup alpha 0.2 (the mixed batch kernel + the SOFT head kernel)
    both      the two together

    python tools/ab_soft_targets.py --batches 256,32
    python tools/ab_soft_targets.py --summarise <prefix of a rocprofv3 --kernel-trace --stats CSV pair>

As tools/ab_clip.py: arms alternate within each trial, a fresh TrainStep is captured per arm and
trial, ``--reps`` replays are timed with device events; one JSON line per batch. ``--summarise``
reads a kernel trace of such a run: dispatches per step of each arm (run lengths of the dispatch
count between consecutive batch launches) and the durations of the batch kernel (mixed / plain)
and of the head kernel (soft / plain).
"""
import argparse
import csv
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ARMS = {"plain": (0.0, 0.0), "smooth": (0.1, 0.0), "mixup": (0.0, 0.2), "both": (0.1, 0.2)}
BATCH = "augment_kernel<"
KERNELS = ("augment_kernel<false>", "augment_kernel<true", "linear_ce_fwd_kernel<true, false>",
           "linear_ce_fwd_kernel<true, true", "linear_ce_fwd_kernel<false, false>",
           "linear_ce_fwd_kernel<false, true")


def summarise(prefix):
    trace = sorted(csv.DictReader(open(prefix + "_kernel_trace.csv")),
                   key=lambda r: int(r["Start_Timestamp"]))
    idx = [i for i, r in enumerate(trace) if BATCH in r["Kernel_Name"]]
    runs = []  # [batch kernel, dispatches per step, consecutive steps]
    for a, b in zip(idx[:-1], idx[1:]):
        name = "mixed" if "augment_kernel<true" in trace[a]["Kernel_Name"] else "plain"
        head = [r["Kernel_Name"] for r in trace[a:b] if "linear_ce_fwd_kernel<" in r["Kernel_Name"]]
        name += "+soft" if any("<true, true" in h or "<false, true" in h for h in head) else ""
        if runs and runs[-1][0] == name and runs[-1][1] == b - a:
            runs[-1][2] += 1
        else:
            runs.append([name, b - a, 1])
    print("dispatches per step (batch kernel + head, dispatches, consecutive steps):")
    for name, n, k in runs:
        if k >= 5:
            print(f"  {name}: {n} x {k}")
    for key in KERNELS:
        rows = [r for r in trace if key in r["Kernel_Name"]]
        if rows:
            us = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows)
            print(f"{key}: {len(us)} launches, median {us[len(us) // 2]:.2f} us, min {us[0]:.2f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,32")
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--summarise", default=None)
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    import torch
    import ddp_amd
    from ddp_amd.data import DeviceLoader, SyntheticCIFAR10
    from ddp_amd.engine import CrossEntropyLoss, TrainStep
    from ddp_amd.models import build
    from ddp_amd.optim import FusedSGD
    arms = a.arms.split(",")
    dev = torch.device("cuda", 0)
    for B in [int(b) for b in a.batches.split(",")]:
        torch.manual_seed(ddp_amd.SEED)
        ds = SyntheticCIFAR10(True)
        loaders = {al: DeviceLoader(ds, B, dev, 1, 0, train=True, cpad=8, mixup_alpha=al)
                   for al in {ARMS[v][1] for v in arms}}
        model = build("vgg11").to(dev)
        opt = FusedSGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        res = {v: [] for v in arms}
        for _ in range(a.trials):
            for v in arms:
                e, al = ARMS[v]
                st = TrainStep(model, opt, CrossEntropyLoss(label_smoothing=e), loaders[al])
                st.warmup(2)
                st.capture()
                for _ in range(3):
                    st.step()
                torch.cuda.synchronize()
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    st.step()
                e1.record()
                torch.cuda.synchronize()
                res[v].append(e0.elapsed_time(e1) / a.reps)
                del st
            torch.cuda.empty_cache()
        med = {v: sorted(t)[len(t) // 2] for v, t in res.items()}
        print(json.dumps({"batch": B, "median_ms": {v: round(m, 4) for v, m in med.items()},
                          "all_ms": {v: [round(x, 4) for x in t] for v, t in res.items()}}),
              flush=True)
        del model, opt, loaders
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
