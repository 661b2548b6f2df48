"""The no-decay mask in the captured VGG-11 training step, in the deterministic-statistics build
(run as a subprocess of tests/test_gpu_no_decay.py with DDP_AMD_DETERMINISTIC=1, after
tests/det_probe.py; prints one JSON line). Batch 8, one step per execution, plain SGD without
momentum, so the step from a fixed state is p - lr (g + wd p) per element.

  * FusedSGD(no_decay="1d") keeps SGD in the backward (``opt_in_bwd``), and that step equals the
    step with DDP_AMD_SGD_IN_BWD=0 (every update in the step's own launch) by torch.equal;
  * at lr 0 no gamma moves;
  * at lr > 0 the masked and the unmasked optimizer agree bit for bit on every tensor with more
    than one dimension, and on every BatchNorm gamma the unmasked one is lr wd gamma lower.
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
LR, WD = 0.01, 0.05


def main():
    import torch
    import ddp_amd
    assert ddp_amd.native().deterministic(), "DDP_AMD_DETERMINISTIC=1 must load the deterministic build"
    from ddp_amd.data import DeviceLoader, SyntheticCIFAR10
    from ddp_amd.engine import CrossEntropyLoss, TrainStep
    from ddp_amd.models import VGG11
    torch.manual_seed(7)
    model = VGG11().cuda()
    from ddp_amd.optim import FusedSGD
    ld = DeviceLoader(SyntheticCIFAR10(True, n=64), 8, "cuda")
    params = list(model.parameters())
    gammas = [i for i, (n, p) in enumerate(model.named_parameters())
              if p.dim() == 1 and bool((p == 1).all())]
    res = {"gammas": len(gammas)}
    snap = None

    def one_step(lr, mask, in_bwd):
        nonlocal snap
        os.environ["DDP_AMD_SGD_IN_BWD"] = "1" if in_bwd else "0"
        opt = FusedSGD(params, lr=lr, momentum=0.0, weight_decay=WD, no_decay=mask)
        a = opt.arena
        if snap is None:
            snap = (a.data.clone(), ld.cursor.clone())
        a.data.copy_(snap[0])
        ld.cursor.copy_(snap[1])
        a.grad.zero_()
        for sp in model.fused_plan():
            sp._packed_version = None
            sp.maybe_pack()
        st = TrainStep(model, opt, CrossEntropyLoss(), ld)
        torch.cuda.synchronize()
        st._body()
        torch.cuda.synchronize()
        return st.opt_in_bwd, [a.data[o:o + n].clone() for o, n in zip(a.offsets, a.numels)]

    bwd, masked = one_step(LR, "1d", True)
    a = params[0]._ddp_amd_arena
    p0 = [snap[0][o:o + n].clone() for o, n in zip(a.offsets, a.numels)]
    res["opt_in_bwd"] = bool(bwd)
    nob, masked_launch = one_step(LR, "1d", False)
    res["launch_only_opt_in_bwd"] = bool(nob)
    res["in_bwd_equals_launch"] = all(torch.equal(x, y) for x, y in zip(masked, masked_launch))
    _, plain = one_step(LR, None, True)
    _, frozen = one_step(0.0, "1d", True)
    res["lr0_gammas_unchanged"] = all(torch.equal(frozen[i], p0[i]) for i in gammas)
    res["weights_equal"] = all(torch.equal(masked[i], plain[i]) for i, p in enumerate(params)
                               if p.dim() > 1)
    res["weights_moved"] = all(not torch.equal(masked[i], p0[i])
                               for i, p in enumerate(params) if p.dim() == 4)
    # gamma is 1.0: p - lr g against p - lr (g + wd p), each a few roundings of values near 1
    shift = [float((masked[i] - plain[i] - LR * WD * p0[i]).abs().max()) for i in gammas]
    res["gamma_shift_err"] = max(shift)
    res["gamma_shift"] = LR * WD
    print(json.dumps(res))


if __name__ == "__main__":
    main()
