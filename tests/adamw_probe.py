"""AdamW inside the training steps (run as a subprocess of tests/test_gpu_adamw.py, a fresh child
per mode: the extension is loaded once per process; prints one JSON line). VGG-11, batch 32, the
shapes of tests/ema_probe.py.

    python tests/adamw_probe.py det     # DDP_AMD_DETERMINISTIC=1: eager == captured over 3 steps,
                                        #   p, m, v (and the EMA): plain, with a cosine schedule,
                                        #   --accum-steps 2 with clipping and the EMA
    python tests/adamw_probe.py count   # dispatches of one replay of the captured b32 step: AdamW,
                                        #   and SGD without SGD in the backward
"""
import copy
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
B, STEPS = 32, 3


class Rig:
    """One model + AdamW + loader with a start state every run returns to."""

    def __init__(self, base, K=1, schedule=None, ema=None, **opt_kw):
        import torch
        from ddp_amd.data import DeviceLoader, SyntheticCIFAR10
        from ddp_amd.engine import CrossEntropyLoss, TrainStep
        from ddp_amd.optim import AdamW
        self.model = copy.deepcopy(base)
        self.opt = AdamW(self.model.parameters(), lr=1e-3, **opt_kw)
        if schedule is not None:
            self.opt.set_schedule(schedule)
        if ema is not None:
            self.opt.set_ema(ema)
        self.ld = DeviceLoader(SyntheticCIFAR10(True, n=B * K * STEPS), B,
                               torch.device("cuda", 0))
        self.arena = self.opt.arena
        self.st = TrainStep(self.model, self.opt, CrossEntropyLoss(), self.ld, accum_steps=K)
        self.st.warmup(2)  # lazy allocations, the fused plan
        torch.cuda.synchronize()
        self.opt.momentum_buffer.zero_()
        self.opt.second_moment.zero_()
        self.opt.set_lr_step(0)
        self.snap = (self.arena.data.clone(), self.opt.state_snapshot())

    def restore(self):
        import torch
        torch.cuda.synchronize()
        self.arena.data.copy_(self.snap[0])
        self.opt.restore_state(self.snap[1])
        self.ld.cursor.zero_()
        self.arena.grad.zero_()
        self.opt.repack()
        torch.cuda.synchronize()

    def run(self, fn):
        import torch
        self.restore()
        for _ in range(STEPS):
            fn()
        torch.cuda.synchronize()
        o = self.opt
        return (self.arena.data.clone(), o.momentum_buffer.clone(), o.second_moment.clone(),
                o.ema.clone() if o.ema_decay is not None else None, o.lr_step,
                o.lr_step_device())


def _base():
    import torch
    from ddp_amd.models import VGG11
    torch.manual_seed(31)
    return VGG11().cuda()


def det_case():
    import torch
    import ddp_amd
    from ddp_amd.optim import LRSchedule
    assert ddp_amd.native().deterministic(), \
        "DDP_AMD_DETERMINISTIC=1 must load the deterministic build"
    base = _base()
    res = {}
    for name, kw in (("plain", {}),
                     ("cosine", dict(schedule=LRSchedule(1e-3, STEPS, warmup_steps=1,
                                                         decay="cosine"))),
                     ("accum2_clip_ema", dict(K=2, max_grad_norm=1e-3, ema=0.9))):
        rig = Rig(base, **kw)
        st = rig.st
        res[f"{name}/opt_in_bwd_off"] = st.opt_in_bwd is False
        eager = rig.run(st._body)
        st.capture()
        res[f"{name}/captured"] = st.graph is not None
        graph = rig.run(st.step)
        for i, what in enumerate(("masters", "m", "v")):
            res[f"{name}/{what}"] = torch.equal(eager[i], graph[i])
        res[f"{name}/ema"] = eager[3] is None or torch.equal(eager[3], graph[3])
        res[f"{name}/t"] = eager[4:] == graph[4:] == (STEPS, STEPS)
        res[f"{name}/moved"] = not torch.equal(eager[0], rig.snap[0])
        res[f"{name}/v_moved"] = bool((eager[2] > 0).any())
        res[f"{name}/cursor"] = int(rig.ld.cursor) == STEPS * kw.get("K", 1)
        if "max_grad_norm" in kw:
            res[f"{name}/clipped"] = float(rig.opt.clip_coef()) < 1.0
    return res


def count_case():
    from ema_probe import Rig as SgdRig, _dispatches
    base = _base()
    res = {}
    os.environ["DDP_AMD_SGD_IN_BWD"] = "0"
    rig = SgdRig(base, ema=False)
    res["sgd_no_in_bwd/opt_in_bwd"] = bool(rig.st.opt_in_bwd)
    res["sgd_no_in_bwd"], res["sgd_no_in_bwd/update_launches"] = _dispatches(rig.st)
    os.environ["DDP_AMD_SGD_IN_BWD"] = "1"
    rig = Rig(base)
    res["adamw/opt_in_bwd"] = bool(rig.st.opt_in_bwd)
    res["adamw"], res["adamw/update_launches"] = _dispatches(rig.st)
    return res


def main():
    res = {"det": det_case, "count": count_case}[sys.argv[1]]()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
