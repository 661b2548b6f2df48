"""LARS on the GPU (optim/lars.py, csrc/kernels/optim.hip chunk_sums_kernel<true> +
sgd_pack_kernel<true, .>): per-tensor trust ratios computed on the device by every launch, eager
and replayed."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ETA, EPS, WD, MOM, GS = 0.02, 1e-8, 1e-4, 0.9, 0.5

# Longest serial chain of rounded additions behind one tensor's sum of squares (all terms are
# non-negative, so a chain of k additions is off by at most k * 2^-24 relative):
#   chunk_sums_kernel   8 float4 iterations x 4 fmas + 1 tail fma per thread        33
#                       wave_sum: 4 DPP levels + 2 levels over the four rows          6
#                       four wave results added serially by thread 0                 3
#   sgd_pack_kernel     lane l adds chunks l, l + 64, ... (<= 64 chunks here)          1
#                       wave_sum                                                     6
CHAIN = 33 + 6 + 3 + 1 + 6
# trust = eta * wn / (gn + wd * wn + eps): the square roots halve each norm's error (CHAIN / 2
# each for numerator and denominator = CHAIN), plus single roundings: two sqrt, eta * wn,
# wd * wn, two additions, the division, and eta as an fp32 argument.
TRUST_RTOL = (CHAIN + 8) * 2.0 ** -24


def _kernel_params():
    """Item kind 1 (channel-padded 3->64 conv, 1728 elements: LDS-tiled re-pack), kind 2
    (64->72 conv, 41,472 elements = 5 chunks + 512: a partial last chunk, a multi-partial sum),
    kind 0 (Linear(33, 10) weight, 330 elements: the scalar tail of the norms kernel; a
    BatchNorm pair and a 33-element vector: 1-D, excluded; a 2-D tensor whose gradient is 0)."""
    from ddp_amd.ops.layers import ConvBNActSpec
    torch.manual_seed(3)
    c0 = torch.nn.Conv2d(3, 64, 3, padding=1).to(DEV)
    b0 = torch.nn.BatchNorm2d(64).to(DEV)
    c1 = torch.nn.Conv2d(64, 72, 3, padding=1).to(DEV)
    lin = torch.nn.Linear(33, 10, bias=False).to(DEV)
    specs = [ConvBNActSpec(c0, b0, cin_pad=8), ConvBNActSpec(c1, None)]
    params = list(c0.parameters()) + list(b0.parameters()) + list(c1.parameters()) + \
        [lin.weight, torch.nn.Parameter(torch.randn(33, device=DEV)),
         torch.nn.Parameter(torch.randn(5, 12, device=DEV))]
    return params, specs


ZERO_GRAD = 8          # index of the 2-D tensor whose gradient stays zero
ADAPTED = (0, 4, 6)    # conv 3->64, conv 64->72, Linear weight


def _grads(params, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    gs = [torch.randn(p.shape, device=DEV, generator=g) for p in params]
    gs[ZERO_GRAD].zero_()
    return gs


def _set_grads(params, gs):
    for p, gr in zip(params, gs):
        p.grad.copy_(gr)


def _copies(specs):
    out = []
    for s in specs:
        out.append(s.wc.clone())
        if s.wt is not None:
            out.append(s.wt.clone())
    return out


class _Table:
    """Schedule stand-in with an explicit table (the optimizer only needs table() / lr_at())."""

    def __init__(self, values):
        self._t = torch.tensor(values, dtype=torch.float32)
        self.total_steps = len(values)

    def table(self):
        return self._t

    def lr_at(self, k):
        return float(self._t[min(max(int(k), 0), self.total_steps - 1)])

    def state_dict(self):
        return {}


def _make(cls, nesterov=False, **kw):
    ps, specs = _kernel_params()
    opt = cls(ps, lr=0.3, momentum=MOM, weight_decay=WD, nesterov=nesterov, grad_scale=GS, **kw)
    return ps, specs, opt


def _lars(**kw):
    from ddp_amd.optim import LARS
    return _make(LARS, trust_coefficient=ETA, eps=EPS, **kw)


def _same(pa, sa, oa, pb, sb, ob):
    for i, (p, q) in enumerate(zip(pa, pb)):
        assert torch.equal(p, q), i
    assert torch.equal(oa.momentum_buffer, ob.momentum_buffer)
    for c, d in zip(_copies(sa), _copies(sb)):
        assert torch.equal(c, d)


def _trust_oracle(params, gs):
    out = []
    for i, (p, g) in enumerate(zip(params, gs)):
        wn = p.detach().double().norm()
        gn = (g.double() * GS).norm()
        ok = p.dim() > 1 and float(wn) > 0 and float(gn) > 0
        out.append(float(ETA * wn / (gn + WD * wn + EPS)) if ok else 1.0)
    return torch.tensor(out, dtype=torch.float64)


@pytest.mark.parametrize("nesterov", [False, True])
def test_trust_ratios_and_update_match_the_oracle(native_ext, nesterov):
    from ddp_amd.optim import LARS
    ps, specs, opt = _lars(nesterov=nesterov)
    kinds = set(int(k) for k in opt._work_table()[0][:, 0].tolist())
    assert kinds == {0, 1, 2}, kinds
    assert [opt.arena.numels[i] for i in ADAPTED] == [1728, 41472, 330]
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    copt = LARS(cpu, lr=0.3, momentum=MOM, weight_decay=WD, nesterov=nesterov, grad_scale=GS,
                trust_coefficient=ETA, eps=EPS)
    for k in range(3):
        gs = _grads(ps, 10 + k)
        want = _trust_oracle(ps, gs)
        _set_grads(ps, gs)
        for p, gr in zip(cpu, gs):
            p.grad = gr.cpu().clone()
        opt.step()
        copt.step()
        torch.cuda.synchronize()
        trust = opt.trust_ratios()
        assert trust.is_cuda and trust.data_ptr() == opt.trust_ratios().data_ptr()
        got = trust.double().cpu()
        err = ((got - want).abs() / want).max()
        print(f"step {k}: trust {got.tolist()} max rel err {float(err):.3e} (bound {TRUST_RTOL:.3e})")
        assert torch.allclose(got, want, rtol=TRUST_RTOL, atol=0.0), (k, got, want)
        for i in range(len(ps)):
            assert (float(got[i]) == 1.0) == (i not in ADAPTED), i
        for i, (p, c) in enumerate(zip(ps, cpu)):
            assert torch.allclose(p.detach().cpu(), c.detach(), rtol=1e-5, atol=1e-6), (k, i)
            buf = opt.arena.shaped(opt.momentum_buffer, i).cpu()
            assert torch.allclose(buf, copt.state[c]["momentum_buffer"], rtol=1e-5, atol=1e-6), (k, i)
        # bf16 operand copies == bf16(new master), exactly
        c0, c1 = ps[0].detach(), ps[4].detach()
        wc0 = specs[0].wc.view(64, 3, 3, 8).float()
        assert torch.equal(wc0[..., :3], c0.permute(0, 2, 3, 1).to(torch.bfloat16).float())
        assert float(wc0[..., 3:].abs().max()) == 0.0
        if specs[0].wt is not None:
            assert torch.equal(specs[0].wt.view(-1, 3, 3, 64)[:3].float(),
                               c0.permute(1, 2, 3, 0).to(torch.bfloat16).float())
        assert torch.equal(specs[1].wc.view(72, 3, 3, 64).float(),
                           c1.permute(0, 2, 3, 1).to(torch.bfloat16).float())


def test_excluded_tensors_take_the_plain_sgd_update_bitwise(native_ext):
    from ddp_amd.optim import FusedSGD
    pa, sa, oa = _lars()
    pb, sb, ob = _make(FusedSGD)
    for k in range(3):
        gs = _grads(pa, 20 + k)
        _set_grads(pa, gs)
        _set_grads(pb, gs)
        oa.step()
        ob.step()
        torch.cuda.synchronize()
        for i in range(len(pa)):
            if i in ADAPTED:
                assert not torch.equal(pa[i], pb[i]), (k, i)
                continue
            assert torch.equal(pa[i], pb[i]), (k, i)
            assert torch.equal(oa.arena.shaped(oa.momentum_buffer, i),
                               ob.arena.shaped(ob.momentum_buffer, i)), (k, i)


def test_two_runs_are_bit_identical(native_ext):
    pa, sa, oa = _lars()
    pb, sb, ob = _lars()
    for k in range(3):
        gs = _grads(pa, 30 + k)
        _set_grads(pa, gs)
        _set_grads(pb, gs)
        oa.step()
        ob.step()
        torch.cuda.synchronize()
        _same(pa, sa, oa, pb, sb, ob)
        assert torch.equal(oa.trust_ratios(), ob.trust_ratios())


def test_ranges_equal_the_whole_arena_step(native_ext):
    """Per-bucket launches (``params=(i0, i1)``): each range runs the norms of its own tensors
    and sums the partials in the same order as the whole-arena launch."""
    pa, sa, oa = _lars()
    pb, sb, ob = _lars()
    n = len(pa)
    for k, cuts in enumerate(([0, 3, 5, n], [0, 1, 4, 7, n])):
        gs = _grads(pa, 40 + k)
        _set_grads(pa, gs)
        _set_grads(pb, gs)
        oa.step(zero_grad=True)
        for i0, i1 in list(zip(cuts[:-1], cuts[1:]))[::-1]:  # last layers first, as the DDP step
            ob.step(params=(i0, i1), zero_grad=True)
        torch.cuda.synchronize()
        _same(pa, sa, oa, pb, sb, ob)
        assert torch.equal(oa.trust_ratios(), ob.trust_ratios())
        assert float(oa.arena.grad.abs().max()) == 0.0 and float(ob.arena.grad.abs().max()) == 0.0


@pytest.mark.parametrize("scheduled", [False, True])
def test_captured_step_equals_eager(native_ext, scheduled):
    pa, sa, oa = _lars()
    pb, sb, ob = _lars()
    table = [0.3, 0.05, 0.2, 0.1]
    if scheduled:
        oa.set_schedule(_Table(table))
        ob.set_schedule(_Table(table))
    # warm up on a side stream (builds every device table), roll the state back, capture
    snap = (oa.arena.data.clone(), oa.momentum_buffer.clone())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _set_grads(pa, _grads(pa, 49))
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
    for k in range(3):
        gs = _grads(pa, 50 + k)
        _set_grads(pa, gs)
        _set_grads(pb, gs)
        graph.replay()
        oa.count_step()
        ob.step(zero_grad=True, lr_advance=True)
        torch.cuda.synchronize()
        _same(pa, sa, oa, pb, sb, ob)
        assert torch.equal(oa.trust_ratios(), ob.trust_ratios())
        assert float(oa.arena.grad.abs().max()) == 0.0
        seen.append(oa.trust_ratios().clone())
    # nothing was baked in at capture: every replay computed its own ratios
    for i in ADAPTED:
        assert len({float(t[i]) for t in seen}) == 3, i
    if scheduled:
        assert oa.lr_step == 3 and oa.lr_step_device() == 3 == ob.lr_step_device()


def test_skip_word_leaves_everything_unchanged(native_ext):
    ps, specs, opt = _lars()
    _set_grads(ps, _grads(ps, 60))
    opt.momentum_buffer.normal_()
    opt.repack()  # the operand copies are written by the first update: give them a value
    before = (opt.arena.data.clone(), opt.momentum_buffer.clone(), _copies(specs))
    err = torch.ones(1, dtype=torch.int32, device=DEV)
    opt.step(zero_grad=True, skip=err.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(opt.arena.data, before[0])
    assert torch.equal(opt.momentum_buffer, before[1])
    for c, d in zip(_copies(specs), before[2]):
        assert torch.equal(c, d)
    err.zero_()
    opt.step(zero_grad=True, skip=err.data_ptr())
    torch.cuda.synchronize()
    assert not torch.equal(opt.arena.data, before[0])


# ------------------------------------------------------------------------------------ engine
LR, E_ETA = 0.5, 0.02


def _engine(ddp):
    from ddp_amd.models import VGG11
    from ddp_amd.engine import CrossEntropyLoss
    from ddp_amd.optim import LARS
    from ddp_amd.data import SyntheticCIFAR10, DeviceLoader
    from ddp_amd.parallel import DistributedDataParallel, RcclCommunicator
    torch.manual_seed(4)
    m = VGG11().cuda()
    if ddp:
        m = DistributedDataParallel(m, RcclCommunicator(0, 1, 0), bucket_cap_mb=256.0,
                                    first_bucket_cap_mb=256.0)
    opt = LARS(m.parameters(), lr=LR, momentum=0.0, weight_decay=0.0, trust_coefficient=E_ETA)
    ld = DeviceLoader(SyntheticCIFAR10(True, n=128), 16, DEV)
    # a conv bias in front of a train-mode BatchNorm has no gradient (the mean removes it): with
    # wd 0 it is the one kind of parameter that a step leaves where it was
    inner = getattr(m, "module", m)
    opt.still = {id(c.bias) for c in inner.layers if isinstance(c, torch.nn.Conv2d)}
    return m, opt, CrossEntropyLoss(), ld


def _check_step(opt, fn, what):
    """Momentum 0, wd 0: |w_new - w_old| / |w_old| = lr * eta / (1 + eps / gn) for every adapted
    tensor, whatever its gradient; a plain SGD update (a WGRAD finish that took the update, a
    missing ratio) misses that by orders of magnitude. rtol 1e-3: fp32 rounding of p gives
    about 6e-6, eps about 1e-6."""
    a = opt.arena
    old = a.data.clone()
    fn()
    torch.cuda.synchronize()
    want = LR * E_ETA
    for i, p in enumerate(a.params):
        o, n = a.offsets[i], a.numels[i]
        w0, w1 = old[o:o + n].double(), a.data[o:o + n].double()
        if id(p) in opt.still:
            continue
        assert not torch.equal(w0, w1), (what, i)
        if float(w0.norm()) == 0.0:  # BatchNorm beta starts at zero: no ratio to take
            continue
        ratio = float((w1 - w0).norm() / w0.norm())
        if p.dim() > 1:
            assert ratio == pytest.approx(want, rel=1e-3), (what, i, tuple(p.shape), ratio)
            assert float(opt.trust_ratios()[i]) != 1.0
        else:
            assert ratio != pytest.approx(want, rel=1e-3), (what, i, tuple(p.shape), ratio)
            assert float(opt.trust_ratios()[i]) == 1.0


def test_train_step_applies_the_trust_ratio(native_ext):
    from ddp_amd.engine import TrainStep
    m, opt, crit, ld = _engine(ddp=False)
    st = TrainStep(m, opt, crit, ld)
    assert st.opt_in_bwd is False
    with pytest.raises(RuntimeError):
        opt.register_in_backward()
    _check_step(opt, st._body, "eager")
    st.warmup(1)
    st.capture()
    torch.cuda.synchronize()
    assert st.graph is not None and st.opt_in_bwd is False
    _check_step(opt, st.step, "replay")
    _check_step(opt, st.step, "replay 2")


def test_segmented_step_applies_the_trust_ratio(native_ext):
    from ddp_amd.engine import SegmentedDDPStep
    m, opt, crit, ld = _engine(ddp=True)
    try:
        for kw in (dict(update="shard16", emulate_world=8), dict(zero=True),
                   dict(update=["ar", "s16", "ar"], emulate_world=8)):
            with pytest.raises(ValueError, match='update="allreduce"'):
                SegmentedDDPStep(m, opt, crit, ld, split=[3, 6], emulate_gbps=171.0, **kw)
        ss = SegmentedDDPStep(m, opt, crit, ld, split=[3, 6], emulate_gbps=171.0)
        ss.WAIT_TIMEOUT_S = 20.0
        assert ss.opt_in_bwd is False and len(ss.buckets) == 3
        _check_step(opt, ss._body, "eager")
        ss.check_error()
        ss.warmup(1)
        ss.capture()
        torch.cuda.synchronize()
        _check_step(opt, ss.step, "replay")
        _check_step(opt, ss.step, "replay 2")
        ss.check_error()
    finally:
        m.close()
