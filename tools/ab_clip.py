#!/usr/bin/env python3
"""What the gradient guard costs on the captured VGG-11 training step (one MI355X), in-process,
three arms on the same build, all with DDP_AMD_SGD_IN_BWD=0 (the guard gives up SGD in the
backward, so the fair baseline is the step whose every update runs in the step's own launch):

    sgd_nobwd    FusedSGD, no guard
    clip_never   + max_grad_norm that is never reached (c == 1: the same update, bit for bit)
    clip_always  + max_grad_norm that always clips

    python tools/ab_clip.py --batches 256,32
    python tools/ab_clip.py --summarise <prefix of a rocprofv3 --kernel-trace --stats CSV pair>

clip_* - sgd_nobwd is the cost of the guard: one sum-of-squares launch over the gradient and the
prologue of the update launch. As tools/ab_lars.py: arms alternate within each trial, a fresh
TrainStep is captured per arm and trial, ``--reps`` replays are timed with device events; one
JSON line per batch. ``--summarise`` reads a kernel trace of such a run: dispatches per step of
each arm (run lengths of the dispatch count between consecutive update launches) and the
sum-of-squares kernel's duration.
"""
import argparse
import csv
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ARMS = ("sgd_nobwd", "clip_never", "clip_always")
# (the synthetic set is memorised within a few hundred steps and the gradient norm falls by
# orders of magnitude: "always" has to stay below any norm the run can reach)
NEVER, ALWAYS = 1e30, 1e-12
# the update launch, optim.hip sgd_pack_kernel<LARS, GUARD, EMA, ADAM>, and the sum-of-squares launch
UPDATE = re.compile(r"sgd_pack_kernel<(true|false), (true|false), (true|false), (true|false)>")
SUMSQ = "chunk_sums_kernel<false>"


def summarise(prefix):
    trace = sorted(csv.DictReader(open(prefix + "_kernel_trace.csv")),
                   key=lambda r: int(r["Start_Timestamp"]))
    idx = [i for i, r in enumerate(trace) if UPDATE.search(r["Kernel_Name"])]
    runs = []  # [update kernel, dispatches per step, consecutive steps]
    for a, b in zip(idx[:-1], idx[1:]):
        guard = UPDATE.search(trace[b]["Kernel_Name"]).group(2) == "true"
        name = "sgd_clip_pack" if guard else "sgd_pack"
        if runs and runs[-1][0] == name and runs[-1][1] == b - a:
            runs[-1][2] += 1
        else:
            runs.append([name, b - a, 1])
    print("dispatches per step (update kernel, dispatches, consecutive steps):")
    for name, n, k in runs:
        if k >= 5:
            print(f"  {name}: {n} x {k}")
    for key in (SUMSQ, "sgd_pack_kernel<false, true, false>", "sgd_pack_kernel<false, false, false>"):
        rows = [r for r in trace if key in r["Kernel_Name"]]
        if rows:
            us = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows)
            wg = int(rows[-1]["Workgroup_Size_X"]) or 1
            blocks = int(rows[-1]["Grid_Size_X"]) // wg
            print(f"{key}: {len(us)} launches, {blocks} blocks, median {us[len(us) // 2]:.2f} us, "
                  f"min {us[0]:.2f} us")


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
    os.environ["DDP_AMD_SGD_IN_BWD"] = "0"
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
        hp = dict(lr=0.01, momentum=0.9, weight_decay=1e-4)
        opts = {"sgd_nobwd": FusedSGD(model.parameters(), **hp),
                "clip_never": FusedSGD(model.parameters(), max_grad_norm=NEVER, **hp),
                "clip_always": FusedSGD(model.parameters(), max_grad_norm=ALWAYS, **hp)}
        crit = CrossEntropyLoss()
        res = {v: [] for v in arms}
        coef = {}
        for _ in range(a.trials):
            for v in arms:
                st = TrainStep(model, opts[v], crit, loader)
                assert st.opt_in_bwd is False
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
                if opts[v].guarded:
                    coef[v] = float(opts[v].clip_coef())
                del st
            torch.cuda.empty_cache()
        assert coef.get("clip_never", 1.0) == 1.0 and coef.get("clip_always", 0.0) < 1.0, coef
        med = {v: sorted(t)[len(t) // 2] for v, t in res.items()}
        print(json.dumps({"batch": B, "elements": sum(p.numel() for p in model.parameters()),
                          "last_clip_coef": coef,
                          "median_ms": {v: round(m, 4) for v, m in med.items()},
                          "all_ms": {v: [round(x, 4) for x in t] for v, t in res.items()}}),
              flush=True)
        del model, opts, loader
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
