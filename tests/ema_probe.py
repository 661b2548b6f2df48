"""Weight EMA inside the training steps (run as a subprocess of tests/test_gpu_ema.py, a fresh
child per mode: the extension is loaded once per process; prints one JSON line). VGG-11, batch
32, decay 0.9, 4 optimizer steps.

    python tests/ema_probe.py det       # DDP_AMD_DETERMINISTIC=1: eager == captured, masters and
                                        #   EMA, plain / --accum-steps 2 / LARS with clipping
    python tests/ema_probe.py release   # the captured step's EMA == the fp32 lerp recurrence over
                                        #   the masters snapshotted after each replay
    python tests/ema_probe.py count     # dispatches of one replay of the captured b32 step: EMA
                                        #   off, EMA on, and EMA off without SGD in the backward
"""
import copy
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
B, STEPS, DECAY = 32, 4, 0.9
HP = dict(lr=0.01, momentum=0.9, weight_decay=1e-4)


class Rig:
    """One model + optimizer + loader with a start state every run returns to (the EMA starts
    as a copy of the start weights)."""

    def __init__(self, base, opt_cls=None, ema=True, K=1, **opt_kw):
        import torch
        from ddp_amd.data import DeviceLoader, SyntheticCIFAR10
        from ddp_amd.engine import CrossEntropyLoss, TrainStep
        from ddp_amd.optim import FusedSGD
        self.model = copy.deepcopy(base)
        self.opt = (opt_cls or FusedSGD)(self.model.parameters(), **dict(HP, **opt_kw))
        if ema:
            self.opt.set_ema(DECAY)
        # (the device with its index, as the mains name it: the loader's launch then clears the
        # model's per-step scratch and the forward needs no fill of its own)
        self.ld = DeviceLoader(SyntheticCIFAR10(True, n=B * K * STEPS), B,
                               torch.device("cuda", 0))
        self.arena = self.opt.arena
        self.st = TrainStep(self.model, self.opt, CrossEntropyLoss(), self.ld, accum_steps=K)
        self.st.warmup(2)  # lazy allocations, the fused plan
        torch.cuda.synchronize()
        self.snap = (self.arena.data.clone(), self.opt.momentum_buffer.clone())

    def restore(self):
        import torch
        torch.cuda.synchronize()
        self.arena.data.copy_(self.snap[0])
        self.opt.momentum_buffer.copy_(self.snap[1])
        if self.opt.ema_decay is not None:
            self.opt.ema.copy_(self.snap[0])
        self.ld.cursor.zero_()
        self.arena.grad.zero_()
        self.opt.repack()
        torch.cuda.synchronize()

    def run(self, fn, each=None):
        import torch
        self.restore()
        for _ in range(STEPS):
            fn()
            if each is not None:
                torch.cuda.synchronize()
                each()
        torch.cuda.synchronize()
        return self.arena.data.clone(), self.opt.ema.clone(), self.opt.momentum_buffer.clone()


def _base():
    import torch
    from ddp_amd.models import VGG11
    torch.manual_seed(31)
    return VGG11().cuda()


def det_case():
    import torch
    import ddp_amd
    from ddp_amd.optim import LARS
    assert ddp_amd.native().deterministic(), \
        "DDP_AMD_DETERMINISTIC=1 must load the deterministic build"
    base = _base()
    res = {}
    for name, kw in (("plain", {}), ("accum2", dict(K=2)),
                     ("lars_clip", dict(opt_cls=LARS, trust_coefficient=0.02,
                                        max_grad_norm=1e-3))):
        rig = Rig(base, **kw)
        st = rig.st
        res[f"{name}/opt_in_bwd_off"] = st.opt_in_bwd is False
        eager = rig.run(st._body)
        st.capture()
        graph = rig.run(st.step)
        res[f"{name}/masters"] = torch.equal(eager[0], graph[0])
        res[f"{name}/ema"] = torch.equal(eager[1], graph[1])
        res[f"{name}/momentum"] = torch.equal(eager[2], graph[2])
        res[f"{name}/moved"] = not torch.equal(eager[0], rig.snap[0])
        res[f"{name}/ema_moved"] = (not torch.equal(eager[1], rig.snap[0])
                                    and not torch.equal(eager[1], eager[0]))
        res[f"{name}/cursor"] = int(rig.ld.cursor) == STEPS * kw.get("K", 1)
        if name == "lars_clip":
            res[f"{name}/clipped"] = float(rig.opt.clip_coef()) < 1.0
    return res


def release_case():
    import torch
    from ddp_amd.optim.sgd import ema_lerp, one_minus_decay
    rig = Rig(_base())
    st = rig.st
    st.capture()
    snaps = []
    got = rig.run(st.step, each=lambda: snaps.append(rig.arena.data.clone()))
    omd = one_minus_decay(DECAY)
    e = rig.snap[0].clone()
    for p in snaps:
        e = ema_lerp(e, p, omd)
    bad = int((e.view(torch.int32) != got[1].view(torch.int32)).sum())
    return {"captured": st.graph is not None, "snapshots": len(snaps) == STEPS,
            "moved": not torch.equal(snaps[0], snaps[-1]),
            "ema_is_the_recurrence": bad == 0, "differing": bad,
            "ema_differs_from_masters": not torch.equal(got[1], got[0])}


def _dispatches(st):
    """Kernel dispatches of one replay of the captured step, from the profiler's device
    activity records (copies and fills are no dispatches); the names go to stderr."""
    import torch
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    st.capture()
    st.step()  # the first replay uploads the graph
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        st.step()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA
             and not re.match(r"(?i)(memcpy|memset|hipmemcpy|hipmemset|copy|fill)", e.name)]
    print(len(names), names, file=sys.stderr)
    return len(names), sum("sgd_pack_kernel" in n for n in names)


def count_case():
    base = _base()
    res = {}
    for name, ema, in_bwd in (("off", False, "1"), ("on", True, "1"), ("off_no_in_bwd", False, "0")):
        os.environ["DDP_AMD_SGD_IN_BWD"] = in_bwd
        rig = Rig(base, ema=ema)
        res[f"{name}/opt_in_bwd"] = bool(rig.st.opt_in_bwd)
        res[name], res[f"{name}/update_launches"] = _dispatches(rig.st)
    return res


def main():
    res = {"det": det_case, "release": release_case, "count": count_case}[sys.argv[1]]()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
