"""Muon inside TrainStep under DDP_AMD_DETERMINISTIC=1 (a fresh child of tests/test_gpu_muon.py: the
extension is loaded once per process; prints one JSON line). VGG-11, batch 32, cosine schedule,
skip_nonfinite and the weight EMA: three steps eager, the same three as replays of the captured
step. The second step finds an Inf in the head's bias, so its gradient is not finite and the
guard skips it INSIDE the step, eager and replayed alike."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
B, STEPS = 32, 3


def main():
    import torch
    import ddp_amd
    from ddp_amd.data import DeviceLoader, SyntheticCIFAR10
    from ddp_amd.engine import CrossEntropyLoss, TrainStep
    from ddp_amd.models import VGG11
    from ddp_amd.optim import LRSchedule, Muon
    assert ddp_amd.native().deterministic(), "DDP_AMD_DETERMINISTIC=1 must load the deterministic build"
    torch.manual_seed(31)
    model = VGG11().cuda()
    opt = Muon(model.parameters(), lr=0.02, weight_decay=1e-4, skip_nonfinite=True)
    opt.set_schedule(LRSchedule(0.02, STEPS, warmup_steps=1, decay="cosine"))
    opt.set_ema(0.9)
    ld = DeviceLoader(SyntheticCIFAR10(True, n=B * STEPS), B, torch.device("cuda", 0))
    st = TrainStep(model, opt, CrossEntropyLoss(), ld)
    st.warmup(2)
    torch.cuda.synchronize()
    a = opt.arena
    opt.momentum_buffer.zero_()
    opt.set_lr_step(0)
    snap = (a.data.clone(), opt.state_snapshot())
    bias0 = a.offsets[-1]  # the head's bias: nothing but the logits reads it
    assert a.params[-1].dim() == 1
    state = lambda: [t.clone() for t in (a.data, opt.momentum_buffer, opt.ema)]  # noqa: E731
    res = {"opt_in_bwd_off": st.opt_in_bwd is False}

    def run(fn, name):
        torch.cuda.synchronize()
        a.data.copy_(snap[0])
        opt.restore_state(snap[1])
        ld.cursor.zero_()
        a.grad.zero_()
        opt.repack()
        skipped = int(opt.skipped_steps())
        for k in range(STEPS):
            if k == 1:
                keep = a.data[bias0].clone()
                a.data[bias0] = float("inf")
                before = state()
            fn()
            torch.cuda.synchronize()
            if k == 1:
                res[f"{name}/skipped_step_untouched"] = all(
                    torch.equal(x, y) for x, y in zip(before, state()))
                a.data[bias0] = keep
        res[f"{name}/skipped_once"] = int(opt.skipped_steps()) - skipped == 1
        res[f"{name}/t"] = (opt.lr_step, opt.lr_step_device()) == (STEPS, STEPS)
        return state()

    eager = run(st._body, "eager")
    st.capture()
    res["captured"] = st.graph is not None
    graph = run(st.step, "graph")
    for what, x, y in zip(("masters", "m", "ema"), eager, graph):
        res[what] = torch.equal(x, y)
    res["moved"] = not torch.equal(eager[0], snap[0]) and bool(torch.isfinite(eager[0]).all())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
