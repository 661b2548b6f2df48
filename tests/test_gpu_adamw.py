"""AdamW (--optimizer adamw, optim/adamw.py) inside the training steps. VGG-11, batch 32 and 16.

* deterministic build (tests/adamw_probe.py, a fresh child: the extension is loaded once per
  process): the eager loop and the captured TrainStep end with torch.equal p, m, v over 3 steps
  -- plain, with a cosine schedule, and with --accum-steps 2, clipping and the EMA (t advances
  once per optimizer step);
* dispatches: the AdamW step has the dispatches of the SGD step without SGD in the backward
  (DDP_AMD_SGD_IN_BWD=0), counted as tests/test_gpu_ema.py counts, and one update launch;
* the captured step's masters follow the oracle's recurrence from the gradients it saw: a copy
  of the gradient arena is captured in front of the update launch, and after every replay p, m, v
  must lie within the kernel's bound (tests/test_gpu_adamw_exact.py) of tests/adamw_oracle.py
  applied to the state before the replay, with the table entry of that step;
* TrainStep and SegmentedDDPStep (emulated collective, world 1) apply it, eager and replayed:
  from a zero state and with wd = 0 the first step moves every element by lr * |G| / (|G| + eps),
  that is by lr wherever the gradient is well above eps and never by more, whatever the gradient's
  size (an SGD update misses that by orders of magnitude): checked on the largest move and on the
  90th percentile of every weight tensor's moves;
* the loss of one batch decreases over 20 captured steps at lr 1e-3.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import adamw_oracle as ao
from exactness import FP32_EPS, assert_within

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
LR = 1e-3


def _probe(case, det=False):
    env = dict(os.environ)
    env.pop("DDP_AMD_SGD_IN_BWD", None)
    env.pop("DDP_AMD_DETERMINISTIC", None)
    if det:
        env["DDP_AMD_DETERMINISTIC"] = "1"
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "adamw_probe.py"), case],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(case, res)
    return res, r.stderr


def test_eager_equals_captured_deterministic(native_ext):
    res, _ = _probe("det", det=True)
    assert len(res) == 3 * 10 + 1
    bad = {k: v for k, v in res.items() if v is not True}
    assert not bad, bad


def test_adamw_has_the_dispatches_of_sgd_without_sgd_in_the_backward(native_ext):
    res, names = _probe("count")
    assert res["adamw/opt_in_bwd"] is False and res["sgd_no_in_bwd/opt_in_bwd"] is False
    assert res["adamw"] == res["sgd_no_in_bwd"], names[-4000:]
    assert res["adamw/update_launches"] == res["sgd_no_in_bwd/update_launches"] == 1


def _engine(ddp, batch=16, **kw):
    from ddp_amd.models import VGG11
    from ddp_amd.engine import CrossEntropyLoss
    from ddp_amd.optim import AdamW
    from ddp_amd.data import SyntheticCIFAR10, DeviceLoader
    from ddp_amd.parallel import DistributedDataParallel, RcclCommunicator
    torch.manual_seed(4)
    m = VGG11().cuda()
    if ddp:
        m = DistributedDataParallel(m, RcclCommunicator(0, 1, 0), bucket_cap_mb=256.0,
                                    first_bucket_cap_mb=256.0)
    opt = AdamW(m.parameters(), lr=LR, **kw)
    ld = DeviceLoader(SyntheticCIFAR10(True, n=128), batch, DEV)
    return m, opt, CrossEntropyLoss(), ld


def _check_first_step(opt, fn, what):
    """Zero state, t = 1, wd = 0: a1 omb1 == 1 and a2 sqrt(omb2) == 1 up to rounding, so
    |dp| = lr |G| / (|G| + eps) <= lr. rtol 1e-3 on lr = 1e-3: the rounding of p (|p| < 4, half an
    ulp 2.4e-7) stays below 2.4e-4 of it, the table roundings and eps far below."""
    a = opt.arena
    torch.cuda.synchronize()
    opt.momentum_buffer.zero_()
    opt.second_moment.zero_()
    opt.set_lr_step(0)
    old = a.data.clone()
    assert float(old.abs().max()) < 4.0
    fn()
    torch.cuda.synchronize()
    assert opt.lr_step == 1 == opt.lr_step_device(), what
    d = (a.data.double() - old.double()).abs()
    assert float(d.max()) <= LR * (1 + 1e-3), (what, float(d.max()))
    for i, p in enumerate(a.params):
        if p.dim() < 2:
            continue
        o, n = a.offsets[i], a.numels[i]
        q90 = float(d[o:o + n].kthvalue(max(1, int(0.9 * n))).values)
        assert q90 == pytest.approx(LR, rel=1e-3), (what, i, tuple(p.shape), q90)
    assert bool((opt.second_moment > 0).any())


def test_train_step_applies_adamw(native_ext):
    from ddp_amd.engine import TrainStep
    m, opt, crit, ld = _engine(ddp=False, weight_decay=0.0)
    st = TrainStep(m, opt, crit, ld)
    assert st.opt_in_bwd is False
    with pytest.raises(RuntimeError, match="AdamW"):
        opt.register_in_backward()
    _check_first_step(opt, st._body, "eager")
    st.warmup(1)
    st.capture()
    torch.cuda.synchronize()
    assert st.graph is not None and st.opt_in_bwd is False
    _check_first_step(opt, st.step, "replay")
    _check_first_step(opt, st.step, "replay 2")


def test_segmented_step_applies_adamw(native_ext):
    from ddp_amd.engine import SegmentedDDPStep
    m, opt, crit, ld = _engine(ddp=True, weight_decay=0.0)
    try:
        for kw in (dict(update="shard16", emulate_world=8), dict(zero=True),
                   dict(update=["ar", "s16", "ar"], emulate_world=8)):
            with pytest.raises(ValueError, match='update="allreduce"'):
                SegmentedDDPStep(m, opt, crit, ld, split=[3, 6], emulate_gbps=171.0, **kw)
        ss = SegmentedDDPStep(m, opt, crit, ld, split=[3, 6], emulate_gbps=171.0)
        ss.WAIT_TIMEOUT_S = 20.0
        assert ss.opt_in_bwd is False and len(ss.buckets) == 3
        _check_first_step(opt, ss._body, "eager")
        ss.check_error()
        ss.warmup(1)
        ss.capture()
        torch.cuda.synchronize()
        _check_first_step(opt, ss.step, "replay")
        _check_first_step(opt, ss.step, "replay 2")
        ss.check_error()
    finally:
        m.close()


def test_captured_masters_follow_the_oracle_recurrence(native_ext):
    """Three replays with a cosine schedule; the gradients each update consumed are copied out by
    a node captured in front of the update launch."""
    from ddp_amd.engine import TrainStep
    from ddp_amd.optim import LRSchedule
    m, opt, crit, ld = _engine(ddp=False, batch=32)
    sched = LRSchedule(LR, 6, warmup_steps=1, decay="cosine", warmup_start_factor=0.25)
    opt.set_schedule(sched)
    st = TrainStep(m, opt, crit, ld)
    st.warmup(1)
    a = opt.arena
    seen = torch.zeros_like(a.grad)
    launch = opt._update_launch

    def recording(*args, **kw):
        seen.copy_(a.grad)
        return launch(*args, **kw)
    opt._update_launch = recording
    st.capture()
    torch.cuda.synchronize()
    assert st.graph is not None
    opt.momentum_buffer.zero_()
    opt.second_moment.zero_()
    opt.set_lr_step(0)
    g = opt.param_groups[0]
    for k in range(3):
        before = [t.cpu().double() for t in (a.data, opt.momentum_buffer, opt.second_moment)]
        st.step()
        torch.cuda.synchronize()
        assert opt.lr_step == k + 1 == opt.lr_step_device()
        a1, a2 = opt.bias_at(k)
        hp = ao.hyper(sched.lr_at(k), g["weight_decay"], opt.grad_scale_factor, *g["betas"],
                      g["eps"], a1, a2)
        grad = seen.cpu().double()
        assert bool(grad.any()) and not bool(a.grad.any())
        want = ao.adamw_ref(before[0], grad, before[1], before[2], hp)
        bd = ao.bounds(ao.adamw_abs(before[0], grad, before[1], before[2], hp), FP32_EPS)
        for name, got, w in (("p", a.data, want[0]), ("m", opt.momentum_buffer, want[1]),
                             ("v", opt.second_moment, want[2])):
            worst = assert_within(got.cpu(), w, bd[name], what=f"replay {k}: {name}")
            print(f"replay {k}: worst |err|/bound {name} {worst:.3f}")
        assert not torch.equal(a.data.cpu().double(), before[0])


def test_loss_decreases_over_20_steps(native_ext):
    """One batch, 20 captured steps at lr 1e-3: the mean loss of the last three steps is below
    that of the first three."""
    from ddp_amd.engine import TrainStep
    m, opt, crit, ld = _engine(ddp=False, batch=32)
    st = TrainStep(m, opt, crit, ld)
    st.warmup(1)
    st.capture()
    torch.cuda.synchronize()
    losses = []
    for _ in range(20):
        ld.cursor.zero_()
        st.loss_sum.zero_()
        st.step()
        torch.cuda.synchronize()
        losses.append(float(st.loss_sum))
    print("losses", [round(v, 4) for v in losses])
    assert all(v == v for v in losses)
    assert sum(losses[-3:]) < sum(losses[:3])
