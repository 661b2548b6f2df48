"""LAMB inside the training steps (run as a subprocess of tests/test_gpu_lamb.py, a fresh child per
mode: the extension is loaded once per process; prints one JSON line). VGG-11, batch 32, the rig
of tests/adamw_probe.py with the optimizer class as a parameter.

    python tests/lamb_probe.py det     # DDP_AMD_DETERMINISTIC=1: eager == captured over 3 steps under
                                       #   a schedule whose rate and t change every step: p, m, v,
                                       #   the ratios; and with --accum-steps 2, clipping, the EMA
    python tests/lamb_probe.py count   # dispatches of one replay of the captured b32 step: LAMB
                                       #   and AdamW
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import adamw_probe as ap  # noqa: E402

STEPS = ap.STEPS


class Rig(ap.Rig):
    """adamw_probe.Rig with ``cls`` in AdamW's place."""

    def __init__(self, base, cls, **kw):
        import ddp_amd.optim as optim
        real = optim.AdamW
        optim.AdamW = cls   # (Rig imports the name from the package when it is built)
        try:
            super().__init__(base, **kw)
        finally:
            optim.AdamW = real
        assert type(self.opt) is cls

    def run(self, fn):
        out = super().run(fn)
        trust = self.opt.trust_ratios().clone() if hasattr(self.opt, "trust_ratios") else None
        return out + (trust,)


def det_case():
    import torch
    import ddp_amd
    from ddp_amd.optim import LAMB, LRSchedule
    assert ddp_amd.native().deterministic(), \
        "DDP_AMD_DETERMINISTIC=1 must load the deterministic build"
    base = ap._base()
    res = {}
    for name, kw in (("cosine", dict(schedule=LRSchedule(2e-3, STEPS, warmup_steps=1,
                                                         decay="cosine"))),
                     ("accum2_clip_ema", dict(K=2, max_grad_norm=1e-3, ema=0.9))):
        rig = Rig(base, LAMB, **kw)
        st = rig.st
        res[f"{name}/opt_in_bwd_off"] = st.opt_in_bwd is False
        eager = rig.run(st._body)
        st.capture()
        res[f"{name}/captured"] = st.graph is not None
        graph = rig.run(st.step)
        for i, what in enumerate(("masters", "m", "v")):
            res[f"{name}/{what}"] = torch.equal(eager[i], graph[i])
        res[f"{name}/ema"] = eager[3] is None or torch.equal(eager[3], graph[3])
        res[f"{name}/t"] = eager[4:6] == graph[4:6] == (STEPS, STEPS)
        res[f"{name}/ratios"] = torch.equal(eager[6], graph[6])
        res[f"{name}/adapted"] = bool((eager[6] != 1.0).any()) and bool((eager[6] == 1.0).any())
        res[f"{name}/moved"] = not torch.equal(eager[0], rig.snap[0])
        if "max_grad_norm" in kw:
            res[f"{name}/clipped"] = float(rig.opt.clip_coef()) < 1.0
    return res


def count_case():
    from ema_probe import _dispatches
    from ddp_amd.optim import AdamW, LAMB
    base = ap._base()
    res = {}
    for name, cls in (("adamw", AdamW), ("lamb", LAMB)):
        rig = Rig(base, cls)
        res[f"{name}/opt_in_bwd"] = bool(rig.st.opt_in_bwd)
        res[name], res[f"{name}/update_launches"] = _dispatches(rig.st)
    return res


def main():
    res = {"det": det_case, "count": count_case}[sys.argv[1]]()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
