#!/usr/bin/env python3
"""What gradient accumulation costs and saves on the captured one-GPU VGG-11 step (one MI355X),
in-process, arms on the same build:

    k1         TrainStep()                        the plain step (SGD in the backward)
    k1_nobwd   the same with DDP_AMD_SGD_IN_BWD=0 every update in the step's own launch
    k2, k4     TrainStep(accum_steps=2 / 4)       accumulated: K micro-batches per replay, one
                                                  update launch (never in the backward)

    python tools/ab_accum.py --batches 256,32
    python tools/ab_accum.py --summarise <prefix of a rocprofv3 --kernel-trace CSV>

As tools/ab_clip.py: arms alternate within each trial, a fresh TrainStep is captured per arm and
trial, ``--reps`` replays are timed with device events and a device synchronize; one JSON line
per batch with the median ms per optimizer step and per micro-batch of every arm and all samples.
``--summarise`` reads a kernel trace of such a run: dispatches per optimizer step (run lengths of
the dispatch count between consecutive update launches).
"""
import argparse
import csv
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ARMS = {"k1": (1, "1"), "k1_nobwd": (1, "0"), "k2": (2, "1"), "k4": (4, "1")}


def summarise(prefix):
    trace = sorted(csv.DictReader(open(prefix + "_kernel_trace.csv")),
                   key=lambda r: int(r["Start_Timestamp"]))
    idx = [i for i, r in enumerate(trace) if "pack_kernel" in r["Kernel_Name"]
           and "pack_conv" not in r["Kernel_Name"]]
    runs = []  # [dispatches per optimizer step, batch launches in it, consecutive steps]
    for a, b in zip(idx[:-1], idx[1:]):
        n_aug = sum("augment_kernel" in r["Kernel_Name"] for r in trace[a + 1:b + 1])
        if runs and runs[-1][0] == b - a and runs[-1][1] == n_aug:
            runs[-1][2] += 1
        else:
            runs.append([b - a, n_aug, 1])
    print("dispatches per optimizer step (dispatches, batch launches, consecutive steps):")
    for n, k, c in runs:
        if c >= 5:
            print(f"  {n} dispatches, K = {k}: x {c}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,32")
    ap.add_argument("--arms", default="k1,k1_nobwd,k2,k4")
    ap.add_argument("--reps", type=int, default=40)
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
        loader = DeviceLoader(SyntheticCIFAR10(True), B, dev, 1, 0, train=True, cpad=8)
        model = build("vgg11").to(dev)
        opt = FusedSGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        crit = CrossEntropyLoss()
        res = {v: [] for v in arms}
        in_bwd = {}
        for _ in range(a.trials):
            for v in arms:
                K, env = ARMS[v]
                os.environ["DDP_AMD_SGD_IN_BWD"] = env
                st = TrainStep(model, opt, crit, loader, accum_steps=K)
                in_bwd[v] = bool(st.opt_in_bwd)
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
                assert float(opt.arena.grad.abs().max()) == 0.0
                del st
            torch.cuda.empty_cache()
        med = {v: sorted(t)[len(t) // 2] for v, t in res.items()}
        print(json.dumps({"batch": B, "sgd_in_backward": in_bwd,
                          "median_ms_per_step": {v: round(m, 4) for v, m in med.items()},
                          "median_ms_per_micro_batch": {v: round(m / ARMS[v][0], 4)
                                                        for v, m in med.items()},
                          "spread_ms": {v: round(max(t) - min(t), 4) for v, t in res.items()},
                          "all_ms": {v: [round(x, 4) for x in t] for v, t in res.items()}}),
              flush=True)
        del model, opt, loader
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
