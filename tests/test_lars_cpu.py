"""LARS on the CPU (optim/lars.py): the class is the oracle of the GPU kernels and the optimizer
of the Gloo paths, so it is checked against a float64 evaluation of the definition itself."""
import pytest
import torch

ETA, EPS, WD, MOM = 0.02, 1e-8, 1e-4, 0.9
SHAPES = [(7, 5), (4, 3, 3, 3), (9,), (6, 4), (3, 8)]
ONE_D, ZERO_GRAD, ZERO_WEIGHT = 2, 3, 4


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]
    with torch.no_grad():
        ps[ZERO_WEIGHT].zero_()
    return ps


def _grads(step):
    g = torch.Generator().manual_seed(100 + step)
    gs = [torch.randn(s, generator=g) for s in SHAPES]
    gs[ZERO_GRAD].zero_()
    return gs


def _reference_step(p, g, buf, lr, nesterov, adapted, gs=1.0):
    """The definition in float64 on one tensor; returns (p, buf, trust)."""
    p, g = p.double(), g.double() * gs
    wn, gn = p.pow(2).sum().sqrt(), g.pow(2).sum().sqrt()
    trust = ETA * wn / (gn + WD * wn + EPS) if (adapted and wn > 0 and gn > 0) else 1.0
    d = trust * (g + WD * p)
    buf = MOM * buf + d
    d = d + MOM * buf if nesterov else buf
    return p - lr * d, buf, float(trust)


@pytest.mark.parametrize("nesterov", [False, True])
def test_cpu_lars_matches_float64_reference(nesterov):
    from ddp_amd.optim import LARS
    lr = 0.3
    ps = _params()
    opt = LARS(ps, lr=lr, momentum=MOM, weight_decay=WD, nesterov=nesterov,
               trust_coefficient=ETA, eps=EPS)
    assert opt.param_groups[0]["exclude_1d"] is True
    ref = [p.detach().double() for p in ps]
    bufs = [torch.zeros_like(r) for r in ref]
    # torch.optim.SGD twins of the tensors whose trust ratio is 1.0 by definition
    twins = {i: torch.nn.Parameter(ps[i].detach().clone()) for i in (ONE_D, ZERO_GRAD, ZERO_WEIGHT)}
    sgd = torch.optim.SGD(list(twins.values()), lr=lr, momentum=MOM, weight_decay=WD,
                          nesterov=nesterov)
    for step in range(3):
        gs = _grads(step)
        # the float64 trajectory runs on its own from the common start
        want = [_reference_step(ref[i], gs[i], bufs[i], lr, nesterov, ps[i].dim() > 1)
                for i in range(len(ps))]
        ref, bufs = [w[0] for w in want], [w[1] for w in want]
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        for i, t in twins.items():
            t.grad = gs[i].clone()
        opt.step()
        sgd.step()
        trust = opt.trust_ratios()
        for i, p in enumerate(ps):
            wp, wb, wt = want[i]
            assert torch.isfinite(p).all() and torch.isfinite(opt.state[p]["momentum_buffer"]).all()
            # fp32 rounds relative to the operands of each add: where terms cancel the floor is
            # 1e-6 of the tensor's largest magnitude, not of the element
            for got, w in ((p.detach(), wp), (opt.state[p]["momentum_buffer"], wb)):
                torch.testing.assert_close(got.double(), w, rtol=1e-6,
                                           atol=1e-6 * float(w.abs().max()))
            assert float(trust[i]) == pytest.approx(wt, rel=1e-6)
        assert float(trust[ONE_D]) == 1.0 and float(trust[ZERO_GRAD]) == 1.0
        assert float(trust[0]) != 1.0 and float(trust[1]) != 1.0
        # excluded / zero-norm tensors: exactly torch.optim.SGD (the zero-weight tensor has a
        # norm of its own after its first update, so only its first step is the plain one)
        for i in (ONE_D, ZERO_GRAD) + ((ZERO_WEIGHT,) if step == 0 else ()):
            assert torch.equal(ps[i].detach(), twins[i].detach()), (step, i)
            assert torch.equal(opt.state[ps[i]]["momentum_buffer"],
                               sgd.state[twins[i]]["momentum_buffer"]), (step, i)
        if step == 0:
            assert float(trust[ZERO_WEIGHT]) == 1.0


def test_exclude_1d_false_adapts_vectors():
    from ddp_amd.optim import LARS
    ps = _params()
    opt = LARS(ps, lr=0.1, trust_coefficient=ETA, exclude_1d=False)
    for p, g in zip(ps, _grads(0)):
        p.grad = g
    w0, g0 = ps[ONE_D].detach().double(), _grads(0)[ONE_D].double()
    opt.step()
    want = ETA * w0.norm() / (g0.norm() + 1e-8)
    assert float(opt.trust_ratios()[ONE_D]) == pytest.approx(float(want), rel=1e-6)


def test_schedule_sets_the_rate_of_step_k():
    """With momentum 0, wd 0 an adapted tensor moves by lr * eta * |w| (1 + O(eps)) in norm:
    the rate a step used can be read back from the update itself."""
    from ddp_amd.optim import LARS, LRSchedule
    sched = LRSchedule(base_lr=0.4, total_steps=4, warmup_steps=2, warmup_start_factor=0.1,
                       decay="cosine")
    table = sched.table()
    assert len(set(float(v) for v in table)) > 2
    ps = _params()
    opt = LARS(ps, lr=9.0, trust_coefficient=ETA)  # the immediate lr is ignored
    opt.set_schedule(sched)
    for k in range(5):  # the fifth step runs on the clamped last entry
        lr = float(table[min(k, 3)])
        assert opt.lr_step == k and opt.current_lr() == lr
        for p, g in zip(ps, _grads(k)):
            p.grad = g
        w0 = ps[0].detach().double().clone()
        opt.step()
        assert opt.param_groups[0]["lr"] == lr
        moved = float((ps[0].detach().double() - w0).norm() / w0.norm())
        assert moved == pytest.approx(lr * ETA, rel=1e-5)
    assert opt.lr_step == 5


def test_checkpoint_round_trip(tmp_path):
    from ddp_amd.optim import LARS
    ps = _params()
    opt = LARS(ps, lr=0.2, momentum=MOM, weight_decay=WD, trust_coefficient=0.05, eps=1e-6,
               exclude_1d=False)
    for p, g in zip(ps, _grads(0)):
        p.grad = g
    opt.step()
    path = str(tmp_path / "opt.pt")
    torch.save(opt.state_dict(), path)
    sd = torch.load(path, weights_only=True)
    g = sd["param_groups"][0]
    assert type(g["trust_coefficient"]) is float and type(g["eps"]) is float
    assert type(g["exclude_1d"]) is bool
    qs = _params(seed=5)
    other = LARS(qs, lr=0.9)
    assert other.param_groups[0]["trust_coefficient"] == 0.001
    other.load_state_dict(sd)
    h = other.param_groups[0]
    assert (h["trust_coefficient"], h["eps"], h["exclude_1d"]) == (0.05, 1e-6, False)
    assert h["lr"] == 0.2 and h["momentum"] == MOM
    for p, q in zip(ps, qs):
        assert torch.equal(opt.state[p]["momentum_buffer"], other.state[q]["momentum_buffer"])
    # same state + same parameters -> the same next step
    with torch.no_grad():
        for p, q in zip(ps, qs):
            q.copy_(p)
    for p, q, gr in zip(ps, qs, _grads(1)):
        p.grad, q.grad = gr.clone(), gr.clone()
    opt.step()
    other.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p, q)


def test_cli_builds_the_optimizer():
    from ddp_amd.optim import FusedSGD, LARS
    from ddp_amd.utils.cli import optimizer_from_args, parse_all
    a = parse_all([], distributed=False)
    assert a.optimizer == "sgd" and a.lars_eta == 0.001 and a.lars_eps == 1e-8
    opt = optimizer_from_args(a, _params(), 0.1)
    assert type(opt) is FusedSGD
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"]) == (0.1, 0.9, 1e-4)
    a = parse_all(["--optimizer", "lars", "--lars-eta", "0.02"], distributed=False)
    opt = optimizer_from_args(a, _params(), 0.8)
    assert type(opt) is LARS
    g = opt.param_groups[0]
    assert g["trust_coefficient"] == 0.02 and g["eps"] == 1e-8 and g["exclude_1d"] is True
    assert (g["lr"], g["momentum"], g["weight_decay"]) == (0.8, 0.9, 1e-4)


def test_refusals():
    from ddp_amd.optim import LARS
    opt = LARS(_params(), lr=0.1)
    with pytest.raises(RuntimeError, match="backward"):
        opt.register_in_backward()
    with pytest.raises(ValueError, match='update="allreduce"'):
        opt.step_elements(0, 64)


def test_gloo_ddp_with_lars():
    from dist_helpers import run_workers
    from lars_dist_worker import ddp_lars_worker
    out = run_workers(ddp_lars_worker, 2, 3, 4)
    for r, v in out.items():
        assert "error" not in v, v.get("error")
        assert v["consistent"] and v["moved"]
        assert 'update="allreduce"' in v["sharded"] and 'update="allreduce"' in v["elements"]
        trust = v["trust"]
        for t, d in zip(trust.tolist(), v["dims"]):
            assert (t == 1.0) == (d == 1), (t, d)
    assert torch.equal(out[0]["params"], out[1]["params"])
    assert torch.equal(out[0]["trust"], out[1]["trust"])
