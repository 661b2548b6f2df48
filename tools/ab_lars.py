#!/usr/bin/env python3
"""What LARS costs on the captured VGG-11 training step (one MI355X), in-process, three arms:

    sgd        FusedSGD, the default step (SGD in the backward where it applies)
    sgd_nobwd  FusedSGD with DDP_AMD_SGD_IN_BWD=0: every update in the step's own launch
    lars       LARS: norms launch + update launch, never in the backward

    python tools/ab_lars.py --batches 256,32
    python tools/ab_lars.py --summarise <prefix of a rocprofv3 --kernel-trace --stats CSV pair>

lars - sgd_nobwd is the cost of the trust ratios; sgd_nobwd - sgd is the known price of giving
up SGD in the backward. As tools/ab_toggle.py: arms alternate within each trial, a fresh
TrainStep is captured per arm and trial, ``--reps`` replays are timed with device events; one
JSON line per batch. ``--summarise`` reads a kernel trace of such a run: dispatches per step of
each arm (run lengths of the dispatch count between consecutive update launches) and the norms
kernel's duration with the bandwidth it implies at 8 bytes per element.
"""
import argparse
import csv
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ARMS = ("sgd", "sgd_nobwd", "lars")
# the update launch, optim.hip sgd_pack_kernel<LARS, GUARD, EMA, ADAM>, and the norms launch
UPDATE = re.compile(r"sgd_pack_kernel<(true|false), (true|false), (true|false), (true|false)>")
NORMS = "chunk_sums_kernel<true>"


def summarise(prefix):
    trace = sorted(csv.DictReader(open(prefix + "_kernel_trace.csv")),
                   key=lambda r: int(r["Start_Timestamp"]))
    idx = [i for i, r in enumerate(trace) if UPDATE.search(r["Kernel_Name"])]
    runs = []  # [update kernel, dispatches per step, consecutive steps]
    for a, b in zip(idx[:-1], idx[1:]):
        lars = UPDATE.search(trace[b]["Kernel_Name"]).group(1) == "true"
        name = "lars_pack" if lars else "sgd_pack"
        if runs and runs[-1][0] == name and runs[-1][1] == b - a:
            runs[-1][2] += 1
        else:
            runs.append([name, b - a, 1])
    print("dispatches per step (update kernel, dispatches, consecutive steps):")
    for name, n, k in runs:
        if k >= 5:
            print(f"  {name}: {n} x {k}")
    norms = [r for r in trace if NORMS in r["Kernel_Name"]]
    if norms:
        us = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in norms)
        wg = int(norms[-1]["Workgroup_Size_X"]) or 1
        blocks = int(norms[-1]["Grid_Size_X"]) // wg
        print(f"{NORMS}: {len(us)} launches, {blocks} blocks, median {us[len(us) // 2]:.2f} us, "
              f"min {us[0]:.2f} us")
    stats = prefix + "_kernel_stats.csv"
    if os.path.exists(stats):
        for r in csv.DictReader(open(stats)):
            if NORMS in r["Name"] or "sgd_pack" in r["Name"]:
                print(f"  stats: {r['Name'][:60]} calls {r['Calls']} avg {float(r['AverageNs']) / 1e3:.2f} us")


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
    from ddp_amd.optim import FusedSGD, LARS
    arms = a.arms.split(",")
    dev = torch.device("cuda", 0)
    for B in [int(b) for b in a.batches.split(",")]:
        torch.manual_seed(ddp_amd.SEED)
        loader = DeviceLoader(SyntheticCIFAR10(True), B, dev, 1, 0, train=True, cpad=8)
        model = build("vgg11").to(dev)
        hp = dict(lr=0.01, momentum=0.9, weight_decay=1e-4)
        sgd = FusedSGD(model.parameters(), **hp)
        opts = {"sgd": sgd, "sgd_nobwd": sgd, "lars": LARS(model.parameters(), **hp)}
        crit = CrossEntropyLoss()
        res = {v: [] for v in arms}
        elements = sum(p.numel() for p in model.parameters() if p.dim() > 1)
        for _ in range(a.trials):
            for v in arms:
                os.environ["DDP_AMD_SGD_IN_BWD"] = "0" if v == "sgd_nobwd" else "1"
                st = TrainStep(model, opts[v], crit, loader)
                assert st.opt_in_bwd == (v == "sgd")
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
        os.environ.pop("DDP_AMD_SGD_IN_BWD", None)
        med = {v: sorted(t)[len(t) // 2] for v, t in res.items()}
        print(json.dumps({"batch": B, "adapted_elements": elements,
                          "median_ms": {v: round(m, 4) for v, m in med.items()},
                          "all_ms": {v: [round(x, 4) for x in t] for v, t in res.items()}}),
              flush=True)
        del model, opts, sgd, loader
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
