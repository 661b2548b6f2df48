"""LAMB (--optimizer lamb, optim/lamb.py) inside the training steps. VGG-11, batch 32 and 16, the
rigs of tests/test_gpu_adamw.py.

* deterministic build (tests/lamb_probe.py, a fresh child): the eager loop and the captured
  TrainStep end with torch.equal p, m, v and ratios over 3 steps under a schedule whose rate and
  t change every step, and with --accum-steps 2, clipping and the EMA;
* dispatches: the LAMB step has AdamW's dispatches plus exactly one per update launch;
* TrainStep and SegmentedDDPStep (stand-in collective, per-bucket launches) apply the ratios,
  eager and replayed: ``trust_ratios()`` after the step matches the fp64 oracle on the gradients
  the step left, within lamb_oracle.trust_rtol, and p follows with the stored ratios;
* the captured step's masters follow the oracle's recurrence over three replays;
* the loss of one batch decreases over 20 captured steps.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import adamw_oracle as ao
import lamb_oracle as lo
from exactness import FP32_EPS, assert_within

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
LR = 2e-3


def _probe(case, det=False):
    env = dict(os.environ)
    env.pop("DDP_AMD_SGD_IN_BWD", None)
    env.pop("DDP_AMD_DETERMINISTIC", None)
    if det:
        env["DDP_AMD_DETERMINISTIC"] = "1"
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "lamb_probe.py"), case],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(case, res)
    return res, r.stderr


def test_eager_equals_captured_deterministic(native_ext):
    res, _ = _probe("det", det=True)
    assert len(res) == 2 * 10 + 1
    bad = {k: v for k, v in res.items() if v is not True}
    assert not bad, bad


def test_lamb_takes_adamws_dispatches_plus_one_per_update_launch(native_ext):
    res, names = _probe("count")
    assert res["lamb/opt_in_bwd"] is False and res["adamw/opt_in_bwd"] is False
    assert res["lamb/update_launches"] == res["adamw/update_launches"] == 1
    assert res["lamb"] == res["adamw"] + res["lamb/update_launches"], names[-4000:]
    assert "lamb_norms_kernel" in names


def _engine(ddp, batch=16, **kw):
    from ddp_amd.models import VGG11
    from ddp_amd.engine import CrossEntropyLoss
    from ddp_amd.optim import LAMB
    from ddp_amd.data import SyntheticCIFAR10, DeviceLoader
    from ddp_amd.parallel import DistributedDataParallel, RcclCommunicator
    torch.manual_seed(4)
    m = VGG11().cuda()
    if ddp:
        m = DistributedDataParallel(m, RcclCommunicator(0, 1, 0), bucket_cap_mb=256.0,
                                    first_bucket_cap_mb=256.0)
    opt = LAMB(m.parameters(), lr=LR, **kw)
    ld = DeviceLoader(SyntheticCIFAR10(True, n=128), batch, DEV)
    return m, opt, CrossEntropyLoss(), ld


class _Recorder:
    """Copies the gradients of a ``step``'s parameter range out in front of it, on the step's
    stream (a captured node when the step is captured): the gradients each update consumed."""

    def __init__(self, opt):
        self.opt, self.seen = opt, torch.zeros_like(opt.arena.grad)
        self.step = opt.step
        opt.step = self

    def __call__(self, *args, **kw):
        a = self.opt.arena
        i0, i1 = kw["params"] if kw.get("params") is not None else (0, len(a.params))
        lo, hi = a.offsets[i0], a.offsets[i1 - 1] + a.numels[i1 - 1]
        stream = kw.get("stream") or torch.cuda.current_stream()
        with torch.cuda.stream(stream):
            self.seen[lo:hi].copy_(a.grad[lo:hi])
        return self.step(*args, **kw)


def _check_step(opt, rec, fn, what, k):
    """One step from the state as it is, table entry ``k``: the ratios against fp64 on the
    recorded gradients, p, m, v against the oracle with the stored ratios."""
    a = opt.arena
    torch.cuda.synchronize()
    opt.set_lr_step(k)
    rec.seen.zero_()
    before = [t.clone() for t in (a.data, opt.momentum_buffer, opt.second_moment)]
    fn()
    torch.cuda.synchronize()
    assert opt.lr_step == k + 1 == opt.lr_step_device(), what
    g = opt.param_groups[0]
    a1, a2 = opt.bias_at(k)
    hp = ao.hyper(opt.schedule.lr_at(k), g["weight_decay"], opt.grad_scale_factor, *g["betas"],
                  g["eps"], a1, a2)
    stored = opt.trust_ratios().cpu()
    assert bool(rec.seen.any()) and not bool(a.grad.any())
    worst_t = 0.0
    for i, prm in enumerate(a.params):
        p, m, v = (a.shaped(t, i).cpu().double().reshape(-1) for t in before)
        gr = a.shaped(rec.seen, i).cpu().double().reshape(-1)
        r = lo.direction(p, gr, m, v, hp)[0]
        T = lo.lamb_abs(p, gr, m, v, hp)
        got_t = float(stored[i])
        if prm.dim() > 1:
            want_t = lo.trust_of(lo.sum_sq(p), lo.sum_sq(r))
            rtol = lo.trust_rtol(r, T["T_r"], FP32_EPS)
            assert abs(got_t - want_t) <= rtol * want_t, (what, i, got_t, want_t, rtol)
            worst_t = max(worst_t, abs(got_t - want_t) / want_t / rtol)
        else:
            assert got_t == 1.0, (what, i)
        want = lo.lamb_ref(p, gr, m, v, hp, trust=got_t)
        bd = lo.bounds(T, FP32_EPS, hp["lr"] * got_t)
        for name, buf, w in (("p", a.data, want[0]), ("m", opt.momentum_buffer, want[1]),
                             ("v", opt.second_moment, want[2])):
            assert_within(a.shaped(buf, i).cpu().reshape(-1), w, bd[name],
                          what=f"{what}: parameter {i}: {name}")
    print(f"{what}: worst ratio error / bound {worst_t:.3f}; ratios "
          f"{[round(float(x), 4) for x in stored[:6]]}")
    assert bool((stored != 1.0).any())


def test_train_step_applies_the_ratios(native_ext):
    from ddp_amd.engine import TrainStep
    m, opt, crit, ld = _engine(ddp=False)
    rec = _Recorder(opt)
    st = TrainStep(m, opt, crit, ld)
    assert st.opt_in_bwd is False
    with pytest.raises(RuntimeError, match="LAMB"):
        opt.register_in_backward()
    _check_step(opt, rec, st._body, "eager", 0)
    st.warmup(1)
    st.capture()
    torch.cuda.synchronize()
    assert st.graph is not None and st.opt_in_bwd is False
    _check_step(opt, rec, st.step, "replay", 1)
    _check_step(opt, rec, st.step, "replay 2", 2)


def test_segmented_step_applies_the_ratios(native_ext):
    from ddp_amd.engine import SegmentedDDPStep
    m, opt, crit, ld = _engine(ddp=True)
    rec = _Recorder(opt)
    try:
        for kw in (dict(update="shard16", emulate_world=8), dict(zero=True),
                   dict(update=["ar", "s16", "ar"], emulate_world=8)):
            with pytest.raises(ValueError, match='LAMB.*update="allreduce"'):
                SegmentedDDPStep(m, opt, crit, ld, split=[3, 6], emulate_gbps=171.0, **kw)
        ss = SegmentedDDPStep(m, opt, crit, ld, split=[3, 6], emulate_gbps=171.0)
        ss.WAIT_TIMEOUT_S = 20.0
        assert ss.opt_in_bwd is False and len(ss.buckets) == 3
        _check_step(opt, rec, ss._body, "eager", 0)
        ss.check_error()
        ss.warmup(1)
        ss.capture()
        torch.cuda.synchronize()
        _check_step(opt, rec, ss.step, "replay", 1)
        _check_step(opt, rec, ss.step, "replay 2", 2)
        ss.check_error()
    finally:
        m.close()


def test_captured_masters_follow_the_oracle_recurrence(native_ext):
    """Three consecutive replays with a cosine schedule, each from the state the last one left."""
    from ddp_amd.engine import TrainStep
    from ddp_amd.optim import LRSchedule
    m, opt, crit, ld = _engine(ddp=False, batch=32)
    opt.set_schedule(LRSchedule(LR, 6, warmup_steps=1, decay="cosine", warmup_start_factor=0.25))
    st = TrainStep(m, opt, crit, ld)
    st.warmup(1)
    rec = _Recorder(opt)
    st.capture()
    torch.cuda.synchronize()
    assert st.graph is not None
    opt.momentum_buffer.zero_()
    opt.second_moment.zero_()
    for k in range(3):
        _check_step(opt, rec, st.step, f"replay {k}", k)


def test_loss_decreases_over_20_steps(native_ext):
    """One batch, 20 captured steps: the mean loss of the last three steps is below that of the
    first three."""
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
