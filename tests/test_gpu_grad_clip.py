"""Gradient clipping and non-finite step skipping on the GPU (optim/sgd.py, optim/lars.py;
csrc/kernels/optim.hip chunk_sums_kernel<false> + sgd_pack_kernel<., true>): norm,
coefficient and verdict are computed on the device by every launch, eager and replayed."""
import pytest
import torch

from test_gpu_lars import (_kernel_params, _grads, _set_grads, _copies, _Table, _same,
                           TRUST_RTOL, ETA, EPS, WD, MOM, GS, ADAPTED)

pytestmark = pytest.mark.gpu
DEV = "cuda"

# Longest serial chain of rounded additions behind the sum of squares of the whole gradient (all
# terms are non-negative, so a chain of k additions is off by at most k * 2^-24 relative):
#   chunk_sums_kernel      8 float4 iterations x 4 fmas + 1 tail fma per thread        33
#                          wave_sum: 4 DPP levels + 2 levels over the four rows          6
#                          four wave results added serially by thread 0                 3
#   clipped update launch  lane l adds chunks l, l + 64, ... (14 chunks here: one each)   1
#                          wave_sum                                                     6
CHAIN = 33 + 6 + 3 + 1 + 6
# the square root halves the error of the sum and rounds once
NORM_RTOL = (CHAIN / 2 + 1) * 2.0 ** -24
# c = max_norm / (norm + eps): the addition, the division, max_norm and eps as fp32 arguments
COEF_RTOL = NORM_RTOL + 4 * 2.0 ** -24
N_CHUNKS = 14


def _make(cls, **kw):
    ps, specs = _kernel_params()
    hp = dict(lr=0.3, momentum=MOM, weight_decay=WD, grad_scale=GS)
    hp.update(kw)
    return ps, specs, cls(ps, **hp)


def _sgd(**kw):
    from ddp_amd.optim import FusedSGD
    return _make(FusedSGD, **kw)


def _norm64(gs, scale=GS):
    return float(torch.sqrt(sum((g.double() * scale).pow(2).sum() for g in gs)))


def _state(opt, specs):
    return (opt.arena.data.clone(), opt.momentum_buffer.clone(), _copies(specs))


def _unchanged(opt, specs, before):
    assert torch.equal(opt.arena.data, before[0])
    assert torch.equal(opt.momentum_buffer, before[1])
    for c, d in zip(_copies(specs), before[2]):
        assert torch.equal(c, d)


def test_norm_and_coefficient_match_fp64_and_the_cpu_twin(native_ext):
    from ddp_amd.optim import FusedSGD
    mx = 20.0
    ps, specs, opt = _sgd(max_grad_norm=mx)
    kinds = set(int(k) for k in opt._work_table()[0][:, 0].tolist())
    assert kinds == {0, 1, 2}, kinds
    assert opt._n_chunks == N_CHUNKS and opt.arena.numels[0] == 1728
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    copt = FusedSGD(cpu, lr=0.3, momentum=MOM, weight_decay=WD, grad_scale=GS, max_grad_norm=mx)
    for k in range(3):
        gs = _grads(ps, 110 + k)
        want = _norm64(gs)
        want_c = min(1.0, mx / (want + 1e-6))
        assert want_c < 0.5
        _set_grads(ps, gs)
        for p, gr in zip(cpu, gs):
            p.grad = gr.cpu().clone()
        opt.step()
        copt.step()
        torch.cuda.synchronize()
        norm = opt.grad_norm()
        assert norm.is_cuda and norm.data_ptr() == opt.grad_norm().data_ptr()
        got, got_c = float(norm), float(opt.clip_coef())
        print(f"step {k}: norm {got!r} (fp64 {want!r}) rel err {abs(got - want) / want:.3e} "
              f"(bound {NORM_RTOL:.3e}); c {got_c!r} rel err {abs(got_c - want_c) / want_c:.3e} "
              f"(bound {COEF_RTOL:.3e})")
        assert abs(got - want) <= NORM_RTOL * want
        assert abs(got_c - want_c) <= COEF_RTOL * want_c
        assert float(copt.grad_norm()) == pytest.approx(want, rel=2.0 ** -23)
        for i, (p, c) in enumerate(zip(ps, cpu)):
            assert torch.allclose(p.detach().cpu(), c.detach(), rtol=1e-5, atol=1e-6), (k, i)
            buf = opt.arena.shaped(opt.momentum_buffer, i).cpu()
            assert torch.allclose(buf, copt.state[c]["momentum_buffer"], rtol=1e-5, atol=1e-6), (k, i)
    assert int(opt.skipped_steps()) == 0


def _pm1(ps, seed):
    """+-1 on exactly 16,384 elements: every element of the eight small tensors (2,415) and
    13,969 of the 64->72 conv weight, its last one among them."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for i, p in enumerate(ps):
        n = p.numel()
        v = (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
        if i == 4:
            keep = torch.zeros(n, dtype=torch.bool)
            keep[torch.randperm(n - 1, generator=g)[:13968]] = True
            keep[n - 1] = True
            v = v * keep
        out.append(v.view(p.shape).to(DEV))
    assert sum(int((o != 0).sum()) for o in out) == 16384
    assert all(float(o.view(-1)[-1]) != 0.0 for o in out)
    return out


@pytest.mark.parametrize("max_norm,equiv_scale", [(16.0, 2.0 ** -3), (64.0, 2.0 ** -1)])
def test_exact_power_of_two_clip_equals_the_rescaled_optimizer(native_ext, max_norm, equiv_scale):
    """grad_scale 2^-1 on 16,384 elements of +-1: S = 4096 and every partial sum is exact,
    norm = 64; max_norm 16, eps 0: c = 2^-2 exactly, the step of grad_scale 2^-3. max_norm 64:
    c = 1, the unclipped step."""
    hp = dict(lr=2.0 ** -2, momentum=2.0 ** -1, weight_decay=2.0 ** -3)
    pa, sa, oa = _sgd(grad_scale=2.0 ** -1, max_grad_norm=max_norm, clip_eps=0.0, **hp)
    pb, sb, ob = _sgd(grad_scale=equiv_scale, **hp)
    assert not ob.guarded
    for k in range(2):
        gs = _pm1(pa, 120 + k)
        _set_grads(pa, gs)
        _set_grads(pb, gs)
        oa.step()
        ob.step()
        torch.cuda.synchronize()
        assert float(oa.grad_norm()) == 64.0
        assert float(oa.clip_coef()) == min(1.0, max_norm / 64.0)
        _same(pa, sa, oa, pb, sb, ob)


def test_ranges_with_one_shared_pass_equal_the_whole_arena_step(native_ext):
    mx = 20.0
    pa, sa, oa = _sgd(max_grad_norm=mx)
    pb, sb, ob = _sgd(max_grad_norm=mx)
    pc, sc, oc = _sgd(max_grad_norm=mx)
    for k in range(2):
        gs = _grads(pa, 130 + k)
        for ps in (pa, pb, pc):
            _set_grads(ps, gs)
        oa.step(zero_grad=True)
        oc.step(zero_grad=True)
        ob.grad_sumsq()
        for rng in ((4, 9), (0, 4)):  # last layers first, as the DDP step
            ob.step(params=rng, zero_grad=True, norm_done=True)
        torch.cuda.synchronize()
        _same(pa, sa, oa, pb, sb, ob)
        _same(pa, sa, oa, pc, sc, oc)  # two runs are bit-identical
        for o in (ob, oc):
            assert torch.equal(oa.grad_norm(), o.grad_norm())
            assert torch.equal(oa.clip_coef(), o.clip_coef())
            assert float(o.arena.grad.abs().max()) == 0.0
        assert float(oa.clip_coef()) < 1.0


def test_nonfinite_step_is_skipped(native_ext):
    table = [0.3, 0.05, 0.2, 0.1, 0.07]
    kw = dict(max_grad_norm=20.0, skip_nonfinite=True)
    pa, sa, oa = _sgd(**kw)
    pb, sb, ob = _sgd(**kw)
    for o in (oa, ob):
        o.set_schedule(_Table(table))
    oa.momentum_buffer.normal_()
    ob.momentum_buffer.copy_(oa.momentum_buffer)
    oa.repack()  # the operand copies are written by the first update: give them a value
    ob.repack()
    cursor = torch.zeros(1, dtype=torch.int32, device=DEV)
    bad_at = ((0, float("nan")), (6, float("inf")))  # kind-1 tensor's last element, kind 0
    for n, (i, bad) in enumerate(bad_at):
        gs = _grads(pa, 140 + n)
        gs[i].view(-1)[-1] = bad
        _set_grads(pa, gs)
        before = _state(oa, sa)
        oa.step(zero_grad=True, counter=(cursor.data_ptr(), 16), lr_advance=True)
        torch.cuda.synchronize()
        _unchanged(oa, sa, before)
        assert float(oa.arena.grad.abs().max()) == 0.0  # (a NaN left behind would show here)
        assert int(cursor) == 16 * (n + 1)
        assert int(oa.skipped_steps()) == n + 1
        assert not torch.isfinite(oa.grad_norm())
        assert oa.lr_step == n + 1 and oa.lr_step_device() == n + 1
    # the finite step that follows equals a twin that never saw the bad ones
    ob.set_lr_step(2)
    gs = _grads(pa, 145)
    _set_grads(pa, gs)
    _set_grads(pb, gs)
    oa.step(zero_grad=True, lr_advance=True)
    ob.step(zero_grad=True, lr_advance=True)
    torch.cuda.synchronize()
    _same(pa, sa, oa, pb, sb, ob)
    assert int(oa.skipped_steps()) == 2 and int(ob.skipped_steps()) == 0
    assert torch.equal(oa.grad_norm(), ob.grad_norm()) and float(oa.clip_coef()) < 1.0
    # the skip word keeps precedence: nothing changes at all, the gradients are not cleared
    gs = _grads(pa, 146)
    gs[4].view(-1)[7] = float("nan")
    _set_grads(pa, gs)
    before = _state(oa, sa)
    stats = oa._guard_dev.clone()
    grad = oa.arena.grad.clone()
    err = torch.ones(1, dtype=torch.int32, device=DEV)
    oa.step(zero_grad=True, skip=err.data_ptr(), lr_advance=True)
    torch.cuda.synchronize()
    _unchanged(oa, sa, before)
    assert torch.equal(oa.arena.grad.view(torch.int32), grad.view(torch.int32))
    assert torch.equal(oa._guard_dev.view(torch.int32), stats.view(torch.int32))
    assert int(oa.skipped_steps()) == 2
    # the options and the count travel with the state_dict (the table stand-in does not)
    oa.set_schedule(None)
    sd = oa.state_dict()
    assert sd["grad_guard"] == {"skipped": 2}
    pc, sc, oc = _sgd()
    assert not oc.guarded and oc.needs_whole_tensors is False
    oc.load_state_dict(sd)
    g = oc.param_groups[0]
    assert (g["max_grad_norm"], g["clip_eps"], g["skip_nonfinite"]) == (20.0, 1e-6, True)
    assert oc.needs_whole_tensors is True and int(oc.skipped_steps()) == 2
    for i in range(len(pa)):
        assert torch.equal(oc.arena.shaped(oc.momentum_buffer, i),
                           oa.arena.shaped(oa.momentum_buffer, i)), i


@pytest.mark.parametrize("scheduled", [False, True])
def test_captured_step_equals_eager(native_ext, scheduled):
    kw = dict(max_grad_norm=100.0, skip_nonfinite=True)  # |randn * GS| is about 105 here
    pa, sa, oa = _sgd(**kw)
    pb, sb, ob = _sgd(**kw)
    table = [0.3, 0.05, 0.2, 0.1, 0.15]
    if scheduled:
        oa.set_schedule(_Table(table))
        ob.set_schedule(_Table(table))
    # warm up on a side stream (builds every device table), roll the state back, capture
    snap = (oa.arena.data.clone(), oa.momentum_buffer.clone())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _set_grads(pa, _grads(pa, 149))
        oa.step(zero_grad=True, lr_advance=True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oa.step(zero_grad=True, lr_advance=True)
    oa.arena.data.copy_(snap[0])
    oa.momentum_buffer.copy_(snap[1])
    oa.arena.grad.zero_()
    oa.set_lr_step(0)
    oa.repack()
    torch.cuda.synchronize()
    seen = []
    for k, what in enumerate(("above", "below", "nonfinite", "above")):
        gs = _grads(pa, 150 + k)
        if what == "below":
            gs = [g * 0.5 for g in gs]
        if what == "nonfinite":
            gs[4].view(-1)[-1] = float("inf")
        _set_grads(pa, gs)
        _set_grads(pb, gs)
        before = _state(oa, sa)
        graph.replay()
        oa.count_step()
        ob.step(zero_grad=True, lr_advance=True)
        torch.cuda.synchronize()
        _same(pa, sa, oa, pb, sb, ob)
        assert torch.equal(oa._guard_dev.view(torch.int32), ob._guard_dev.view(torch.int32))
        assert float(oa.arena.grad.abs().max()) == 0.0
        if what == "nonfinite":
            _unchanged(oa, sa, before)
        else:
            assert not torch.equal(oa.arena.data, before[0])
        c = float(oa.clip_coef())
        assert {"above": c < 1.0, "below": c == 1.0, "nonfinite": c == 0.0}[what], (what, c)
        seen.append(c)
    # nothing was baked in at capture: every replay computed its own coefficient
    assert len(set(seen)) == 4, seen
    assert int(oa.skipped_steps()) == 1
    if scheduled:
        assert oa.lr_step == 4 and oa.lr_step_device() == 4 == ob.lr_step_device()


def test_lars_clips_first(native_ext):
    from ddp_amd.optim import LARS
    mx = 20.0
    lk = dict(trust_coefficient=ETA, eps=EPS)
    ps, specs, opt = _make(LARS, max_grad_norm=mx, clip_eps=0.0, **lk)
    pp, sp, plain = _make(LARS, **lk)
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    copt = LARS(cpu, lr=0.3, momentum=MOM, weight_decay=WD, grad_scale=GS, max_grad_norm=mx,
                clip_eps=0.0, **lk)
    for k in range(3):
        gs = _grads(ps, 160 + k)
        c = min(1.0, mx / _norm64(gs))
        want = []
        for p, g in zip(ps, gs):
            wn, gn = p.detach().double().norm(), (g.double() * GS).norm()
            ok = p.dim() > 1 and float(wn) > 0 and float(gn) > 0
            want.append(float(ETA * wn / (c * gn + WD * wn + EPS)) if ok else 1.0)
        want = torch.tensor(want, dtype=torch.float64)
        _set_grads(ps, gs)
        _set_grads(pp, gs)
        for p, gr in zip(cpu, gs):
            p.grad = gr.cpu().clone()
        opt.step()
        plain.step()
        copt.step()
        torch.cuda.synchronize()
        got = opt.trust_ratios().double().cpu()
        rtol = TRUST_RTOL + COEF_RTOL
        err = ((got - want).abs() / want).max()
        print(f"step {k}: c {float(opt.clip_coef())!r} trust {got.tolist()} max rel err "
              f"{float(err):.3e} (bound {rtol:.3e})")
        assert torch.allclose(got, want, rtol=rtol, atol=0.0), (k, got, want)
        for i in ADAPTED:  # clipping shrinks the gradient norm: a larger ratio than without
            assert float(got[i]) > float(plain.trust_ratios()[i]) * 2.0, i
        for i, (p, q) in enumerate(zip(ps, cpu)):
            assert torch.allclose(p.detach().cpu(), q.detach(), rtol=1e-5, atol=1e-6), (k, i)


# ------------------------------------------------------------------------------------ engine
LR = 0.5


def _engine(ddp, max_norm):
    from ddp_amd.models import VGG11
    from ddp_amd.engine import CrossEntropyLoss
    from ddp_amd.optim import FusedSGD
    from ddp_amd.data import SyntheticCIFAR10, DeviceLoader
    from ddp_amd.parallel import DistributedDataParallel, RcclCommunicator
    torch.manual_seed(4)
    m = VGG11().cuda()
    if ddp:
        m = DistributedDataParallel(m, RcclCommunicator(0, 1, 0), bucket_cap_mb=256.0,
                                    first_bucket_cap_mb=256.0)
    opt = FusedSGD(m.parameters(), lr=LR, momentum=0.0, weight_decay=0.0, max_grad_norm=max_norm,
                   skip_nonfinite=True)
    ld = DeviceLoader(SyntheticCIFAR10(True, n=128), 16, DEV)
    return m, opt, CrossEntropyLoss(), ld


def _moved(opt, fn):
    """2-norm of one step's update over the whole arena (the padding never moves)."""
    old = opt.arena.data.clone()
    fn()
    torch.cuda.synchronize()
    return float((opt.arena.data.double() - old.double()).norm())


def _check_step(opt, fn, what, max_norm):
    """Momentum 0, wd 0: the update is lr * c * g with |c * g| = max_norm / (1 + eps / norm), so
    its 2-norm is lr * max_norm whatever the gradient; an unclipped or per-bucket-clipped update
    misses that by orders of magnitude. rel 1e-3: fp32 rounding of p (2^-24 |w| against
    lr * max_norm) and eps / norm are both far below it at max_norm 1e-3."""
    moved = _moved(opt, fn)
    print(f"{what}: |update| {moved:.6e} want {LR * max_norm:.6e} norm {float(opt.grad_norm()):.4e} "
          f"c {float(opt.clip_coef()):.4e}")
    assert moved == pytest.approx(LR * max_norm, rel=1e-3), what
    assert 0.0 < float(opt.clip_coef()) < 1e-1 and int(opt.skipped_steps()) == 0


def test_train_step_clips_the_whole_update(native_ext):
    from ddp_amd.engine import TrainStep
    mx = 1e-3
    m, opt, crit, ld = _engine(False, mx)
    st = TrainStep(m, opt, crit, ld)
    assert st.opt_in_bwd is False
    with pytest.raises(RuntimeError):
        opt.register_in_backward()
    _check_step(opt, st._body, "eager", mx)
    st.warmup(1)
    st.capture()
    torch.cuda.synchronize()
    assert st.graph is not None and st.opt_in_bwd is False
    _check_step(opt, st.step, "replay", mx)
    _check_step(opt, st.step, "replay 2", mx)


def test_train_step_with_an_unreachable_threshold_does_not_clip(native_ext):
    from ddp_amd.engine import TrainStep
    m, opt, crit, ld = _engine(False, 1e30)
    st = TrainStep(m, opt, crit, ld)
    assert st.opt_in_bwd is False
    moved = _moved(opt, st._body)
    assert float(opt.clip_coef()) == 1.0
    assert moved == pytest.approx(LR * float(opt.grad_norm()), rel=1e-3)
    assert moved > 100 * LR * 1e-3  # orders of magnitude away from the clipped update


def test_segmented_step_clips_with_one_update_launch(native_ext, monkeypatch):
    from ddp_amd.engine import SegmentedDDPStep
    mx = 1e-3
    m, opt, crit, ld = _engine(True, mx)
    calls = {"sgd_pack": 0, "grad_sumsq": 0}
    for name in calls:
        real = getattr(native_ext, name)

        def counted(*a, _real=real, _name=name, **kw):
            calls[_name] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(native_ext, name, counted)
    try:
        for kw in (dict(update="shard16", emulate_world=8), dict(zero=True),
                   dict(update=["ar", "s16", "ar"], emulate_world=8)):
            with pytest.raises(ValueError, match='update="allreduce"'):
                SegmentedDDPStep(m, opt, crit, ld, split=[3, 6], emulate_gbps=171.0, **kw)
        ss = SegmentedDDPStep(m, opt, crit, ld, split=[3, 6], emulate_gbps=171.0)
        ss.WAIT_TIMEOUT_S = 20.0
        assert ss.opt_in_bwd is False and len(ss.buckets) == 3
        _check_step(opt, ss._body, "eager", mx)
        assert calls == {"sgd_pack": 1, "grad_sumsq": 3}, calls  # the launch log of one step
        ss.check_error()
        ss.warmup(1)
        ss.capture()
        torch.cuda.synchronize()
        for k in range(2):
            calls.update(sgd_pack=0, grad_sumsq=0)
            _check_step(opt, ss.step, f"replay {k}", mx)
            assert calls == {"sgd_pack": 1, "grad_sumsq": 3}, calls
        ss.check_error()
    finally:
        m.close()
