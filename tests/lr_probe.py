"""Bitwise learning-rate-schedule comparisons in the deterministic-statistics build (run as a
subprocess of tests/test_gpu_lr_schedule.py with DDP_AMD_DETERMINISTIC=1; prints one JSON line).

    python tests/lr_probe.py single      # TrainStep (SGD in the backward active)
    python tests/lr_probe.py segmented   # SegmentedDDPStep, cuts 3,6, one rank, no collective

Each case trains 6 steps of a warm-up + cosine schedule three ways from the same state: eager
steps with the HOST setting ``param_groups[0]["lr"] = float(table[k])`` and no schedule attached
(the immediate-lr kernels), the captured step with the schedule in device memory (one capture,
six replays), and the same with a re-capture after three replays (the epoch boundary of
engine/apps.py). In this build a step is a deterministic function of its inputs, so the fp32
arena and the momentum buffer must be torch.equal.
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STEPS = 6


def main():
    import torch
    import ddp_amd
    assert ddp_amd.native().deterministic(), "DDP_AMD_DETERMINISTIC=1 must load the det build"
    from ddp_amd.models import VGG11
    from ddp_amd.optim import FusedSGD, LRSchedule
    from ddp_amd.data import SyntheticCIFAR10, DeviceLoader
    from ddp_amd.engine import TrainStep, SegmentedDDPStep, CrossEntropyLoss
    from ddp_amd.parallel import DistributedDataParallel, RcclCommunicator
    case = sys.argv[1]
    torch.manual_seed(11)
    sched = LRSchedule(0.02, STEPS, warmup_steps=2, warmup_start_factor=0.25, decay="cosine")
    table = sched.table()
    if case == "single":
        m = VGG11().cuda()
        opt = FusedSGD(m.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
        ld = DeviceLoader(SyntheticCIFAR10(True, n=512), 64, "cuda")
        st = TrainStep(m, opt, CrossEntropyLoss(), ld)
        arena, plan = opt.arena, m.fused_plan
    else:
        m = DistributedDataParallel(VGG11().cuda(), RcclCommunicator(0, 1, 0),
                                    bucket_cap_mb=256.0, first_bucket_cap_mb=256.0)
        opt = FusedSGD(m.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
        ld = DeviceLoader(SyntheticCIFAR10(True, n=512), 64, "cuda")
        st = SegmentedDDPStep(m, opt, CrossEntropyLoss(), ld, split=[3, 6])
        st.WAIT_TIMEOUT_S = 20.0
        arena, plan = m.arena, m.module.fused_plan
    st.warmup(1)  # lazy allocations, fused plan
    torch.cuda.synchronize()
    snap = (arena.data.clone(), opt.momentum_buffer.clone(), ld.cursor.clone())

    def restore():
        torch.cuda.synchronize()
        arena.data.copy_(snap[0])
        opt.momentum_buffer.copy_(snap[1])
        ld.cursor.copy_(snap[2])
        arena.grad.zero_()
        for sp in plan():
            sp._packed_version = None
            sp.maybe_pack()
        opt.set_lr_step(0)
        torch.cuda.synchronize()

    def result():
        torch.cuda.synchronize()
        if hasattr(st, "check_error"):
            st.check_error()
        return arena.data.clone(), opt.momentum_buffer.clone()

    res = {}
    # 1) eager, the host sets the learning rate, nothing attached
    restore()
    for k in range(STEPS):
        opt.param_groups[0]["lr"] = float(table[k])
        st._body()
    eager = result()
    res["eager_moved"] = bool(float((eager[0] - snap[0]).norm()) > 0)
    opt.param_groups[0]["lr"] = 123.0  # the immediate value must be ignored from here on

    # 2) one capture with the schedule in device memory, six replays
    opt.set_schedule(sched)
    st.warmup(1)
    st.capture()
    restore()
    lrs = []
    for k in range(STEPS):
        lrs.append(opt.current_lr())
        st.step()
    graph = result()
    res["mirror_lrs_match_table"] = lrs == [float(v) for v in table]
    res["graph_equals_eager/arena"] = torch.equal(graph[0], eager[0])
    res["graph_equals_eager/momentum"] = torch.equal(graph[1], eager[1])
    res["graph_step_word"] = opt.lr_step_device() == STEPS and opt.lr_step == STEPS
    if case == "single":
        res["sgd_in_backward_active"] = bool(opt._fused_in_backward() | opt._master_in_backward())

    # 3) re-capture after three replays: the step word carries on
    restore()
    for k in range(3):
        st.step()
    torch.cuda.synchronize()
    st.capture()
    res["recapture_keeps_step_word"] = opt.lr_step_device() == 3 and opt.lr_step == 3
    for k in range(3):
        st.step()
    again = result()
    res["recapture_equals_eager/arena"] = torch.equal(again[0], eager[0])
    res["recapture_equals_eager/momentum"] = torch.equal(again[1], eager[1])
    res["recapture_step_word"] = opt.lr_step_device() == STEPS and opt.lr_step == STEPS
    res["maxdiff"] = float((graph[0] - eager[0]).abs().max())
    if hasattr(m, "close"):
        m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
