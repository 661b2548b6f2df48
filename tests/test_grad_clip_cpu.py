"""Gradient clipping and non-finite step skipping on the CPU (optim/sgd.py, optim/lars.py): the
CPU classes are the oracle of the GPU kernels and the optimizers of the Gloo paths, so they are
checked against torch's own ``clip_grad_norm_`` + ``optim.SGD`` and against the definition."""
import pytest
import torch

MOM, WD = 0.9, 1e-4
# the tensors of tests/test_gpu_lars.py::_kernel_params: conv 3->64 (+ bias, BatchNorm pair),
# conv 64->72 (+ bias), Linear(33, 10) weight, a 33-vector, a 5 x 12 matrix
SHAPES = [(64, 3, 3, 3), (64,), (64,), (64,), (72, 64, 3, 3), (72,), (10, 33), (33,), (5, 12)]


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]


def _pm1_grads(seed):
    """+-1 on 900 elements of the 3->64 conv weight and on 1600 of the 64->72 one, 0 elsewhere:
    per-tensor norms 30 and 40, total 50."""
    g = torch.Generator().manual_seed(seed)
    out = [torch.zeros(s) for s in SHAPES]
    for i, n in ((0, 900), (4, 1600)):
        flat = out[i].view(-1)
        idx = torch.randperm(flat.numel(), generator=g)[:n]
        flat[idx] = (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
    return out


def _rand_grads(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in SHAPES]


def _set(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = g.clone()


@pytest.mark.parametrize("nesterov", [False, True])
def test_clipped_step_equals_torch_clip_grad_norm_bitwise(nesterov):
    from ddp_amd.optim import FusedSGD
    ps, qs = _params(), _params()
    opt = FusedSGD(ps, lr=0.1, momentum=MOM, weight_decay=WD, nesterov=nesterov,
                   max_grad_norm=12.5)
    assert opt.needs_whole_tensors is True and opt.guarded
    ref = torch.optim.SGD(qs, lr=0.1, momentum=MOM, weight_decay=WD, nesterov=nesterov)
    for step in range(2):
        gs = _pm1_grads(step)
        _set(ps, gs)
        _set(qs, gs)
        total = torch.nn.utils.clip_grad_norm_(qs, 12.5)
        assert float(total) == 50.0  # 50 + 1e-6 rounds to 50 in fp32: the coefficient is 0.25
        ref.step()
        opt.step()
        assert float(opt.grad_norm()) == 50.0 and float(opt.clip_coef()) == 0.25
        for i, (p, q) in enumerate(zip(ps, qs)):
            assert torch.equal(p, q), (step, i)
            assert torch.equal(opt.state[p]["momentum_buffer"], ref.state[q]["momentum_buffer"])
    assert int(opt.skipped_steps()) == 0


def test_norm_below_the_threshold_is_the_unclipped_step():
    from ddp_amd.optim import FusedSGD
    ps, qs = _params(), _params()
    opt = FusedSGD(ps, lr=0.1, momentum=MOM, weight_decay=WD, max_grad_norm=50.5)
    plain = FusedSGD(qs, lr=0.1, momentum=MOM, weight_decay=WD)
    assert plain.needs_whole_tensors is False and not plain.guarded
    assert "max_grad_norm" not in plain.param_groups[0]
    for step in range(2):
        gs = _pm1_grads(step)
        _set(ps, gs)
        _set(qs, gs)
        opt.step()
        plain.step()
        assert float(opt.clip_coef()) == 1.0 and float(opt.grad_norm()) == 50.0
        for p, q in zip(ps, qs):
            assert torch.equal(p, q)
            assert torch.equal(opt.state[p]["momentum_buffer"], plain.state[q]["momentum_buffer"])


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_nonfinite_step_is_skipped(bad):
    from ddp_amd.optim import FusedSGD, LRSchedule
    ps, qs = _params(), _params()
    kw = dict(lr=9.0, momentum=MOM, weight_decay=WD, max_grad_norm=1.0, skip_nonfinite=True)
    opt, twin = FusedSGD(ps, **kw), FusedSGD(qs, **kw)
    for o in (opt, twin):
        o.set_schedule(LRSchedule(base_lr=0.4, total_steps=6, warmup_steps=3, decay="cosine"))
    g0 = _rand_grads(0)
    _set(ps, g0)
    _set(qs, g0)
    opt.step(zero_grad=True)
    twin.step(zero_grad=True)
    before = [(p.detach().clone(), opt.state[p]["momentum_buffer"].clone()) for p in ps]
    gb = _rand_grads(1)
    gb[4].view(-1)[-1] = bad
    _set(ps, gb)
    assert opt.lr_step == 1
    opt.step(zero_grad=True)
    for p, (w, b) in zip(ps, before):
        assert torch.equal(p, w) and torch.equal(opt.state[p]["momentum_buffer"], b)
        assert float(p.grad.abs().max()) == 0.0
    assert int(opt.skipped_steps()) == 1 and int(twin.skipped_steps()) == 0
    assert opt.lr_step == 2  # a skipped update still counts as a step
    assert not torch.isfinite(opt.grad_norm())
    # the next finite step: a twin that never saw the bad one, its schedule one step further
    twin.set_lr_step(2)
    g2 = _rand_grads(2)
    _set(ps, g2)
    _set(qs, g2)
    opt.step(zero_grad=True)
    twin.step(zero_grad=True)
    assert opt.current_lr() == twin.current_lr()
    for p, q in zip(ps, qs):
        assert torch.equal(p, q)
        assert torch.equal(opt.state[p]["momentum_buffer"], twin.state[q]["momentum_buffer"])
    assert int(opt.skipped_steps()) == 1


def test_overflowing_sum_counts_as_nonfinite_and_unguarded_arithmetic_is_visible():
    from ddp_amd.optim import FusedSGD
    ps = _params()
    opt = FusedSGD(ps, lr=0.1, max_grad_norm=1.0, skip_nonfinite=True)
    gs = [torch.zeros(s) for s in SHAPES]
    gs[0].fill_(3e19)  # finite elements, sum of squares beyond fp32
    _set(ps, gs)
    w = [p.detach().clone() for p in ps]
    opt.step()
    assert int(opt.skipped_steps()) == 1 and all(torch.equal(p, v) for p, v in zip(ps, w))
    # without skip_nonfinite the coefficient is what the arithmetic says: 0 for Inf, NaN for NaN
    qs = _params()
    o2 = FusedSGD(qs, lr=0.1, max_grad_norm=1.0)
    _set(qs, gs)
    o2.step()
    assert float(o2.clip_coef()) == 0.0 and int(o2.skipped_steps()) == 0
    gs[0].view(-1)[0] = float("nan")
    _set(qs, gs)
    o2.step()
    assert torch.isnan(o2.clip_coef()) and torch.isnan(qs[0]).any()


def test_lars_clips_first():
    """Trust ratios with clipping: eta * wn / (c * gn + wd * wn + eps), c from the norm of the
    whole scaled gradient; the tolerance of tests/test_lars_cpu.py."""
    from ddp_amd.optim import LARS
    eta, eps, gsc, mx = 0.02, 1e-8, 0.5, 3.0
    ps = _params()
    opt = LARS(ps, lr=0.3, momentum=MOM, weight_decay=WD, grad_scale=gsc, trust_coefficient=eta,
               eps=eps, max_grad_norm=mx, clip_eps=0.0)
    plain = LARS(_params(), lr=0.3, momentum=MOM, weight_decay=WD, grad_scale=gsc,
                 trust_coefficient=eta, eps=eps)
    for step in range(3):
        gs = _rand_grads(10 + step)
        total = torch.sqrt(sum((g.double() * gsc).pow(2).sum() for g in gs))
        c = min(1.0, mx / float(total))
        assert c < 0.1
        want = []
        for p, g in zip(ps, gs):
            wn, gn = p.detach().double().norm(), (g.double() * gsc).norm()
            want.append(float(eta * wn / (c * gn + WD * wn + eps)) if p.dim() > 1 else 1.0)
        w0 = [p.detach().double().clone() for p in ps]
        _set(ps, gs)
        _set(plain.param_groups[0]["params"], gs)
        opt.step()
        plain.step()
        assert float(opt.grad_norm()) == pytest.approx(float(total), rel=1e-6)
        assert float(opt.clip_coef()) == pytest.approx(c, rel=1e-6)
        for i, t in enumerate(opt.trust_ratios().tolist()):
            assert t == pytest.approx(want[i], rel=1e-6), (step, i)
            if ps[i].dim() > 1:
                assert t != pytest.approx(float(plain.trust_ratios()[i]), rel=1e-3)
        if step == 0:  # momentum buffer still zero: the first update is lr * trust * (c gs g + wd w)
            for i, (p, g) in enumerate(zip(ps, gs)):
                d = want[i] * (c * gsc * g.double() + WD * w0[i])
                torch.testing.assert_close(p.detach().double(), w0[i] - 0.3 * d, rtol=1e-6,
                                           atol=1e-6 * float(w0[i].abs().max()))


def test_state_dict_round_trip(tmp_path):
    from ddp_amd.optim import FusedSGD, LARS
    ps = _params()
    opt = FusedSGD(ps, lr=0.2, momentum=MOM, weight_decay=WD, max_grad_norm=2.5, clip_eps=1e-3,
                   skip_nonfinite=True)
    gs = _rand_grads(0)
    _set(ps, gs)
    opt.step()
    gs[6].view(-1)[3] = float("nan")
    for _ in range(2):
        _set(ps, gs)
        opt.step()
    assert int(opt.skipped_steps()) == 2
    path = str(tmp_path / "opt.pt")
    torch.save(opt.state_dict(), path)
    sd = torch.load(path, weights_only=True)
    g = sd["param_groups"][0]
    assert (g["max_grad_norm"], g["clip_eps"], g["skip_nonfinite"]) == (2.5, 1e-3, True)
    assert sd["grad_guard"] == {"skipped": 2}
    qs = _params(seed=5)
    other = FusedSGD(qs, lr=0.9)
    assert not other.guarded and other.needs_whole_tensors is False
    other.load_state_dict(sd)
    h = other.param_groups[0]
    assert (h["max_grad_norm"], h["clip_eps"], h["skip_nonfinite"]) == (2.5, 1e-3, True)
    assert other.guarded and other.needs_whole_tensors is True
    assert int(other.skipped_steps()) == 2 and h["lr"] == 0.2
    with torch.no_grad():
        for p, q in zip(ps, qs):
            q.copy_(p)
    g1 = _rand_grads(1)
    _set(ps, g1)
    _set(qs, g1)
    opt.step()
    other.step()
    assert float(other.clip_coef()) < 1.0
    for p, q in zip(ps, qs):
        assert torch.equal(p, q)
    # a plain optimizer's state_dict carries none of it
    plain = FusedSGD(_params(), lr=0.1).state_dict()
    assert "grad_guard" not in plain and "max_grad_norm" not in plain["param_groups"][0]
    # LARS takes the same options
    lars = LARS(_params(), lr=0.1, max_grad_norm=4.0, skip_nonfinite=True)
    sd = lars.state_dict()
    l2 = LARS(_params(), lr=0.1)
    l2.load_state_dict(sd)
    assert l2.param_groups[0]["max_grad_norm"] == 4.0 and l2.guarded
    assert l2.param_groups[0]["trust_coefficient"] == 0.001


def test_refusals():
    from ddp_amd.optim import FusedSGD
    for kw in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True)):
        opt = FusedSGD(_params(), lr=0.1, **kw)
        assert opt.needs_whole_tensors is True
        with pytest.raises(RuntimeError, match="backward"):
            opt.register_in_backward()
        with pytest.raises(ValueError, match='update="allreduce"'):
            opt.step_elements(0, 64)
    with pytest.raises(ValueError):
        FusedSGD(_params(), lr=0.1, max_grad_norm=0.0)
    assert FusedSGD.needs_whole_tensors is False  # the flag is the instance's


def test_cli_flags():
    from ddp_amd.optim import FusedSGD, LARS
    from ddp_amd.utils.cli import optimizer_from_args, parse_all
    a = parse_all([], distributed=False)
    assert a.clip_grad_norm is None and a.skip_nonfinite_grads is False
    opt = optimizer_from_args(a, _params(), 0.1)
    assert type(opt) is FusedSGD and not opt.guarded and opt.needs_whole_tensors is False
    assert "max_grad_norm" not in opt.param_groups[0]
    a = parse_all(["--clip-grad-norm", "2.5", "--skip-nonfinite-grads"], distributed=False)
    opt = optimizer_from_args(a, _params(), 0.1)
    g = opt.param_groups[0]
    assert type(opt) is FusedSGD and opt.guarded
    assert (g["max_grad_norm"], g["clip_eps"], g["skip_nonfinite"]) == (2.5, 1e-6, True)
    a = parse_all(["--optimizer", "lars", "--clip-grad-norm", "1.5"], distributed=False)
    opt = optimizer_from_args(a, _params(), 0.1)
    g = opt.param_groups[0]
    assert type(opt) is LARS and (g["max_grad_norm"], g["skip_nonfinite"]) == (1.5, False)
    a = parse_all(["--skip-nonfinite-grads"], distributed=False)
    opt = optimizer_from_args(a, _params(), 0.1)
    assert opt.guarded and opt.param_groups[0]["max_grad_norm"] is None


def test_metrics_fields():
    from ddp_amd.engine.trainer import _guard_stats
    from ddp_amd.optim import FusedSGD
    assert _guard_stats(FusedSGD(_params(), lr=0.1)) == {}
    ps = _params()
    opt = FusedSGD(ps, lr=0.1, max_grad_norm=12.5)
    _set(ps, _pm1_grads(0))
    opt.step()
    assert _guard_stats(opt) == {"grad_norm": 50.0, "clip_coef": 0.25, "skipped": 0}


@pytest.mark.parametrize("strategy", ["ddp", "allreduce"])
def test_gloo_replicas_stay_identical(strategy):
    from dist_helpers import run_workers
    from grad_clip_dist_worker import clip_worker, MAX_NORM
    out = run_workers(clip_worker, 2, strategy, 3, 4)
    for r, v in out.items():
        assert "error" not in v, v.get("error")
        assert v["skipped"] == 0 and len(v["norms"]) == 3
        for n, c in zip(v["norms"], v["coefs"]):
            assert n > MAX_NORM and c == pytest.approx(MAX_NORM / n, rel=1e-5)
        if strategy == "ddp":
            assert v["consistent"]
            assert 'update="allreduce"' in v["sharded"] and 'update="allreduce"' in v["elements"]
    assert out[0]["norms"] == out[1]["norms"] and out[0]["coefs"] == out[1]["coefs"]
    assert (out[0]["params"] == out[1]["params"]).all()
