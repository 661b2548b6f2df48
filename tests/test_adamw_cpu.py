"""AdamW on the CPU (optim/adamw.py, utils/cli.py, engine, mains, checkpoints): the CPU class is
the oracle of the update kernel's ADAM instantiations and the optimizer of the Gloo paths. The
rule and its oracle: tests/adamw_oracle.py."""
import copy
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import adamw_oracle as ao
from exactness import FP32_EPS, assert_within, int_tensor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 6, 3, padding=1), torch.nn.BatchNorm2d(6),
                               torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(6 * 8 * 8, 5))


def _backward(model, step, scale=1.0):
    g = torch.Generator().manual_seed(100 + step)
    x, y = torch.randn(4, 3, 8, 8, generator=g), torch.randint(0, 5, (4,), generator=g)
    (scale * torch.nn.functional.cross_entropy(model(x), y)).backward()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------- the bias table
def test_bias_table_entries_are_fp64_values_rounded_once():
    from ddp_amd.optim.adamw import bias_table
    t = bias_table(0.9, 0.999)
    k = np.arange(1, len(t) + 1, dtype=np.float64)
    assert np.array_equal(t[:, 0], (1.0 / (1.0 - 0.9 ** k)).astype(np.float32))
    assert np.array_equal(t[:, 1], (1.0 / np.sqrt(1.0 - 0.999 ** k)).astype(np.float32))
    assert t.dtype == np.float32 and t.shape[1] == 2
    # a few entries against exact rational arithmetic: a1 is within half an fp32 ulp of it
    for j in (0, 1, 9, 99):
        exact = 1 / (1 - Fraction(0.9) ** (j + 1))
        a1 = Fraction(float(t[j, 0]))
        assert abs(a1 - exact) <= exact * Fraction(1, 2 ** 24)
    assert t[0, 0] == np.float32(1.0 / (1.0 - 0.9)) and t[0, 1] == np.float32(1.0 / np.sqrt(1.0 - 0.999))


def test_bias_table_is_cut_at_the_first_pair_of_ones():
    from ddp_amd.optim.adamw import bias_table
    for b1, b2, about in ((0.9, 0.999, 16000), (0.9, 0.5, 160), (0.0, 0.0, 1), (0.5, 0.9, 160)):
        t = bias_table(b1, b2)
        one = (t[:, 0] == 1.0) & (t[:, 1] == 1.0)
        assert one[-1] and not one[:-1].any(), (b1, b2)
        assert 0.9 * about <= len(t) <= 1.1 * about + 1, (b1, b2, len(t))
    assert abs(len(bias_table(0.9, 0.999)) - 16000) < 500
    assert abs(len(bias_table(0.9, 0.0)) - 160) < 10


def test_bias_clamp_is_exact_beyond_the_table():
    """Every step beyond the table would compute exactly (1.0f, 1.0f): the clamp loses nothing."""
    from ddp_amd.optim import AdamW
    opt = AdamW(_model().parameters(), betas=(0.9, 0.99))
    n = len(opt.bias)
    assert opt.bias_at(n - 1) == (1.0, 1.0) == opt.bias_at(n) == opt.bias_at(10 * n)
    for t in (n + 1, 2 * n, 100 * n):
        a1, a2 = ao.bias64(0.9, 0.99, t)
        assert np.float32(a1) == 1.0 and np.float32(a2) == 1.0
    assert opt.bias_at(0) == tuple(float(np.float32(x)) for x in ao.bias64(0.9, 0.99, 1))


def test_unreasonable_betas_are_refused():
    from ddp_amd.optim import AdamW
    from ddp_amd.optim.adamw import bias_table
    with pytest.raises(ValueError, match="beta2"):
        bias_table(0.9, 0.9999999)
    with pytest.raises(ValueError, match="beta1"):
        AdamW(_model().parameters(), betas=(0.99999999, 0.999))
    for bad in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999)):
        with pytest.raises(ValueError, match="beta"):
            AdamW(_model().parameters(), betas=bad)
    with pytest.raises(ValueError):
        AdamW(_model().parameters(), eps=-1.0)
    with pytest.raises(ValueError):
        AdamW(_model().parameters(), weight_decay=-1.0)


# ------------------------------------------------------------------------------------ the rule
def test_crafted_state_is_exact_and_the_cpu_path_returns_it():
    """The exact-mode state of tests/test_gpu_adamw_exact.py, 100k elements: the oracle asserts
    that no intermediate rounds, and the CPU path (fp32 tensors, fma32) returns its bits."""
    from ddp_amd.optim import AdamW
    n = 100_000
    g = int_tensor((n,), 1, 64, 1) * (2 * int_tensor((n,), 0, 1, 2) - 1)
    a = int_tensor((n,), 1, 3, 3) * (2 * int_tensor((n,), 0, 1, 4) - 1)
    b = 2.0 ** int_tensor((n,), 0, 2, 5)
    p0 = int_tensor((n,), -64, 64, 6)
    m0, v0 = (2 * a - 1) * g, (2 * b * b - 1) * g * g
    hp = dict(lr=2.0 ** -2, wd=2.0 ** -3, grad_scale=0.5, omb1=0.5, beta2=0.5, omb2=0.5, eps=0.0,
              a1=2.0, a2=0.5)
    want = ao.adamw_ref(p0, 2 * g, m0, v0, hp, exact=True)
    assert torch.equal(want[1], (a * g).double()) and torch.equal(want[2], (b * b * g * g).double())
    p = torch.nn.Parameter(p0.clone())
    opt = AdamW([p], lr=2.0 ** -2, betas=(0.5, 0.5), eps=0.0, weight_decay=2.0 ** -3,
                grad_scale=0.5)
    opt._bias = np.array([[2.0, 0.5]], dtype=np.float32)   # the test's own table
    opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    p.grad = 2 * g
    opt.step()
    st = opt.state[p]
    for name, got, w in (("p", p, want[0]), ("m", st["exp_avg"], want[1]),
                         ("v", st["exp_avg_sq"], want[2])):
        assert torch.equal(_bits(got), _bits(w.float())), name


def test_cpu_path_against_real_arithmetic():
    """AdamW on the CPU against torch.optim.AdamW run in fp64 on the same fp32 inputs, per
    element, after step 1 and after step 3. Hyper-parameters that are fp32 numbers, so both sides
    get the same values: lr 2**-10, betas (1 - 2**-3, 1 - 2**-8), eps 2**-27, wd 2**-7.

    The bound, first order in eps = 2**-24, every count an integer number of roundings. One step
    from exact inputs, with T_m = |m| + omb1 (|G| + |m|):
      G = fl(g gs)                    1 rounding, relative
      d = fl(G - m)                   |err| <= eps |G| + eps (|G| + |m|)
      m' = fma(omb1, d, m)            |err| <= omb1 eps (2 |G| + |m|) + eps T_m <= 3 eps T_m
      w = fl(omb2 G)                  2 eps relative; w G: 3 eps; fl(beta2 v): 1 eps
      v' = fma(w, G, .)               terms >= 0: max(3, 1) + 1 = 4 eps relative
      den = fma(sqrt(v'), a2, eps)    sqrt halves 4 to 2, + 1 (sqrt) + 1 (fma) = 4 eps relative,
                                      + 1 for the table's rounding of a2: 5
      u = fl(m' / den)                (3 + 4 + 1) eps T_m / den = 8, with the a2 rounding 9
      lw = fl(lr wd), q = fma(-lw, p, p)   eps lw |p| + eps (1 + lw) |p| <= eps (1 + 2 lw) |p|
      la = fl(lr a1)                  1 eps relative, + 1 for the table's rounding of a1
      p' = fma(-la, u, q)             la (8 + 1 + 1 + 1) eps T_m / den + eps (1 + 2 lw) |p|
                                      + eps ((1 + lw) |p| + la T_m / den)
                                   <= eps (3 (1 + lw) |p| + 12 la T_m / den)
    Over k steps the inputs carry the earlier steps' errors, all with factors <= 1:
      E_m(k) = E_m(k-1) + 3 eps T_m(k);   v: 4 + 2 (k - 1) eps relative (each step adds the fma's
      and at most one more on the larger term), so den: 5 + (k - 1);
      E_u(k) = (E_m(k) + (5 + (k - 1) + 1) eps T_m(k)) / den(k)
      E_p(k) = E_p(k-1) + eps 3 (1 + lw) |p| + la (E_u(k) + 3 eps T_m(k) / den(k))
    which is the 12 above at k = 1. Magnitudes are taken from the fp64 run."""
    from ddp_amd.optim import AdamW
    lr, b1, b2, eps, wd = 2.0 ** -10, 1 - 2.0 ** -3, 1 - 2.0 ** -8, 2.0 ** -27, 2.0 ** -7
    model = _model(3)
    ps = list(model.parameters())
    ref = [torch.nn.Parameter(p.detach().double().clone()) for p in ps]
    opt = AdamW(ps, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    topt = torch.optim.AdamW(ref, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    E_m = [torch.zeros_like(r) for r in ref]
    E_p = [torch.zeros_like(r) for r in ref]
    worst, T1 = {}, {}
    for k in range(1, 4):
        opt.zero_grad()
        _backward(model, k)
        a1, a2 = opt.bias_at(k - 1)
        hp = ao.hyper(lr, wd, 1.0, b1, b2, eps, a1, a2)
        for i, (p, r) in enumerate(zip(ps, ref)):
            r.grad = p.grad.double().clone()   # the same fp32 gradients on both sides
            st = topt.state.get(r, {})
            m = st.get("exp_avg", torch.zeros_like(r))
            v = st.get("exp_avg_sq", torch.zeros_like(r))
            T = ao.adamw_abs(r.detach(), r.grad, m, v, hp)
            T1.setdefault(i, T)
            E_m[i] = E_m[i] + 3 * FP32_EPS * T["T_m"]
            E_u = (E_m[i] + (5 + (k - 1) + 1) * FP32_EPS * T["T_m"]) / T["den"]
            E_p[i] = E_p[i] + FP32_EPS * 3 * (1 + T["lw"]) * T["p"] + \
                T["la"] * (E_u + 3 * FP32_EPS * T["T_u"])
        opt.step()
        topt.step()
        if k in (1, 3):
            for i, (p, r) in enumerate(zip(ps, ref)):
                w = assert_within(p.detach(), r.detach(), E_p[i], what=f"step {k}: parameter {i}")
                worst[k] = max(worst.get(k, 0.0), w)
                if k == 1:   # the one-step bound of the issue: 12 roundings on the update term
                    one = ao.bounds(T1[i], FP32_EPS, table_roundings=2)["p"]
                    assert bool((E_p[i] <= one * (1 + 1e-12)).all())
    print("worst |err| / bound:", worst)
    assert opt.lr_step == 3
    assert all(float(topt.state[r]["step"]) == 3 for r in ref)


def test_cpu_path_is_within_the_kernels_bound_of_the_oracle():
    """Default hyper-parameters, a history in m and v, t = 3: the CPU path against
    ``adamw_ref`` with the same table entry, within the kernel's bound (10 roundings on the
    update term: the oracle reads the same table)."""
    from ddp_amd.optim import AdamW
    gen = torch.Generator().manual_seed(9)
    n = 20_000
    p0, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    m0, v0 = 0.1 * torch.randn(n, generator=gen), 0.02 * torch.rand(n, generator=gen) + 1e-6
    p = torch.nn.Parameter(p0.clone())
    opt = AdamW([p], grad_scale=0.5)
    opt.set_lr_step(2)
    opt.state[p] = {"step": torch.tensor(2.0), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    p.grad = g.clone()
    opt.step()
    a1, a2 = opt.bias_at(2)
    hp = ao.hyper(1e-3, 1e-2, 0.5, 0.9, 0.999, 1e-8, a1, a2)
    want = ao.adamw_ref(p0, g, m0, v0, hp)
    bd = ao.bounds(ao.adamw_abs(p0, g, m0, v0, hp), FP32_EPS)
    st = opt.state[p]
    for name, got, w in (("p", p, want[0]), ("m", st["exp_avg"], want[1]),
                         ("v", st["exp_avg_sq"], want[2])):
        worst = assert_within(got.detach(), w, bd[name], what=name)
        assert worst > 0.0
    assert opt.lr_step == 3


# -------------------------------------------------------------------------------- the step number
def test_a_skipped_step_still_advances_t():
    from ddp_amd.optim import AdamW
    model = _model()
    opt = AdamW(model.parameters(), skip_nonfinite=True)
    opt.set_ema(0.9)
    _backward(model, 0)
    opt.step()
    assert opt.lr_step == 1 and int(opt.skipped_steps()) == 0
    before = [p.detach().clone() for p in model.parameters()]
    state = [{k: v.clone() for k, v in opt.state[p].items()} for p in model.parameters()]
    ema = opt.ema.clone()
    opt.zero_grad()
    _backward(model, 1)
    next(model.parameters()).grad[0, 0, 0, 0] = float("inf")
    opt.step(zero_grad=True)
    assert opt.lr_step == 2 and int(opt.skipped_steps()) == 1   # t follows the schedule
    for p, b, s in zip(model.parameters(), before, state):
        assert torch.equal(p, b) and not bool(p.grad.any())
        assert torch.equal(opt.state[p]["exp_avg"], s["exp_avg"])
        assert torch.equal(opt.state[p]["exp_avg_sq"], s["exp_avg_sq"])
    assert torch.equal(opt.ema, ema)
    # the next step is taken with the table entry of t = 3
    _backward(model, 2)
    p0 = next(model.parameters())
    old = (p0.detach().clone(), p0.grad.clone(), opt.state[p0]["exp_avg"].clone(),
           opt.state[p0]["exp_avg_sq"].clone())
    opt.step()
    a1, a2 = opt.bias_at(2)
    hp = ao.hyper(1e-3, 1e-2, 1.0, 0.9, 0.999, 1e-8, a1, a2)
    want = ao.adamw_ref(*old, hp)
    bd = ao.bounds(ao.adamw_abs(*old, hp), FP32_EPS)
    assert_within(p0.detach(), want[0], bd["p"], what="step 3 after a skipped step 2")
    a1w, a2w = opt.bias_at(1)
    wrong = ao.adamw_ref(*old, dict(hp, a1=a1w, a2=a2w))[0]
    assert bool(((p0.detach().double() - wrong).abs() > bd["p"]).any())


def test_an_accumulated_step_advances_t_once():
    """Two backward passes, one step at grad_scale 1/2 (what --accum-steps 2 does): one advance,
    and the update of the mean gradient."""
    from ddp_amd.engine.trainer import grad_scaled
    from ddp_amd.optim import AdamW
    model, twin = _model(), _model()
    opt, topt = AdamW(model.parameters(), max_grad_norm=1e3), AdamW(twin.parameters())
    for j in range(2):
        _backward(model, j)
        _backward(twin, j, scale=0.5)
    with grad_scaled(opt, 2):
        opt.step()
    topt.step()
    assert opt.lr_step == 1 == topt.lr_step
    for p, q in zip(model.parameters(), twin.parameters()):
        assert torch.allclose(p, q, rtol=0, atol=2e-6)   # |dp| <= lr = 1e-3, u to a few 1e-4
        assert float(opt.state[p]["step"]) in (0.0, 1.0)
    assert all(float(s["step"]) == 1.0 for s in opt.state_dict()["state"].values())


def test_set_schedule_none_keeps_the_counter():
    from ddp_amd.optim import AdamW, LRSchedule
    model = _model()
    opt = AdamW(model.parameters(), lr=1e-3)
    assert opt.schedule is not None and opt.current_lr() == float(np.float32(1e-3))
    for k in range(2):
        opt.zero_grad()
        _backward(model, k)
        opt.step()
    assert opt.lr_step == 2
    opt.set_schedule(LRSchedule(0.5, 10, decay="linear"), step=2)
    assert opt.lr_step == 2 and opt.current_lr() == LRSchedule(0.5, 10, decay="linear").lr_at(2)
    opt.zero_grad()
    _backward(model, 2)
    opt.step()
    assert opt.lr_step == 3
    opt.param_groups[0]["lr"] = 0.25
    opt.set_schedule(None)
    assert opt.lr_step == 3 and opt.schedule is not None and opt.current_lr() == 0.25
    opt.zero_grad()
    _backward(model, 3)
    opt.step()
    assert opt.lr_step == 4 and opt.current_lr() == 0.25   # the table's last entry, t counts on


# ------------------------------------------------------------------------------- checkpoints
def _trained(steps=2, **kw):
    from ddp_amd.optim import AdamW
    model = _model()
    opt = AdamW(model.parameters(), **kw)
    for k in range(steps):
        opt.zero_grad()
        _backward(model, k)
        opt.step()
    return model, opt


def test_state_dict_round_trip_and_resume_continues_t(tmp_path):
    from ddp_amd.optim import AdamW
    model, opt = _trained(2, betas=(0.8, 0.99), eps=1e-6, max_grad_norm=5.0)
    opt.set_ema(0.9)
    sd = opt.state_dict()
    g = sd["param_groups"][0]
    assert tuple(g["betas"]) == (0.8, 0.99) and g["eps"] == 1e-6 and g["amsgrad"] is False
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert all(float(s["step"]) == 2.0 for s in sd["state"].values())
    path = str(tmp_path / "opt.pt")
    torch.save(sd, path)
    sd = torch.load(path, weights_only=True)
    twin = _model()
    twin.load_state_dict(model.state_dict())
    other = AdamW(twin.parameters())
    other.load_state_dict(sd)
    assert other.lr_step == 2 and other.param_groups[0]["betas"] == (0.8, 0.99)
    assert other.param_groups[0]["eps"] == 1e-6 and other.guarded and other.ema_decay == 0.9
    assert np.array_equal(other.bias, opt.bias)
    other.load_ema_state(opt.ema_state())
    for o, m in ((opt, model), (other, twin)):
        o.zero_grad()
        _backward(m, 5)
        o.step()
    assert other.lr_step == 3
    for p, q in zip(model.parameters(), twin.parameters()):
        assert torch.equal(_bits(p), _bits(q))
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(_bits(opt.state[p][k]), _bits(other.state[q][k]))
    assert torch.equal(opt.ema, other.ema)


def test_a_torch_adamw_state_dict_loads():
    from ddp_amd.optim import AdamW
    model, twin = _model(), _model()
    topt = torch.optim.AdamW(model.parameters(), lr=2e-3, betas=(0.85, 0.98), eps=1e-7,
                             weight_decay=0.05)
    for k in range(3):
        topt.zero_grad()
        _backward(model, k)
        topt.step()
    twin.load_state_dict(model.state_dict())
    opt = AdamW(twin.parameters())
    opt.load_state_dict(copy.deepcopy(topt.state_dict()))   # (torch hands out its own tensors)
    g = opt.param_groups[0]
    assert opt.lr_step == 3 and tuple(g["betas"]) == (0.85, 0.98) and g["eps"] == 1e-7
    assert g["weight_decay"] == 0.05 and opt.current_lr() == float(np.float32(2e-3))
    for p, q in zip(model.parameters(), twin.parameters()):
        assert torch.equal(topt.state[p]["exp_avg_sq"], opt.state[q]["exp_avg_sq"])
    for o, m in ((topt, model), (opt, twin)):   # step 4 on both: the same update, fp32 apart
        o.zero_grad()
        _backward(m, 7)
        o.step()
    assert opt.lr_step == 4
    for p, q in zip(model.parameters(), twin.parameters()):
        assert torch.allclose(p, q, rtol=0, atol=1e-6)   # |dp| <= about lr = 2e-3, fp32 roundings
        assert not torch.equal(p, torch.zeros_like(p))


def test_a_plain_fused_sgd_state_dict_is_unchanged():
    from ddp_amd.optim import FusedSGD
    model = _model()
    opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
    ref = torch.optim.SGD(_model().parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
    _backward(model, 0)
    opt.step()
    sd, rd = opt.state_dict(), ref.state_dict()
    assert set(sd) == {"state", "param_groups"}
    assert set(sd["param_groups"][0]) == set(rd["param_groups"][0])
    assert all(set(s) == {"momentum_buffer"} for s in sd["state"].values())
    assert opt.schedule is None and opt.updates_in_launch_only is False
    assert opt.launch_only_reason is None


# --------------------------------------------------------------------------------------- CLI
def test_cli_defaults_and_weight_decay():
    from ddp_amd.optim import AdamW, FusedSGD, LARS
    from ddp_amd.utils.cli import build_parser, optimizer_from_args
    args = build_parser().parse_args([])
    assert (args.optimizer, args.lr, args.weight_decay) == ("sgd", 0.1, None)
    assert (args.adam_beta1, args.adam_beta2, args.adam_eps) == (0.9, 0.999, 1e-8)
    opt = optimizer_from_args(args, _model().parameters(), args.lr)
    g = opt.param_groups[0]
    assert type(opt) is FusedSGD and (g["lr"], g["momentum"], g["weight_decay"]) == (0.1, 0.9, 1e-4)
    assert "betas" not in g and opt.schedule is None
    lars = optimizer_from_args(build_parser().parse_args(["--optimizer", "lars"]),
                               _model().parameters(), 0.1)
    assert type(lars) is LARS and lars.param_groups[0]["weight_decay"] == 1e-4
    args = build_parser().parse_args(["--optimizer", "adamw", "--lr", "0.001"])
    opt = optimizer_from_args(args, _model().parameters(), args.lr)
    g = opt.param_groups[0]
    assert type(opt) is AdamW and g["weight_decay"] == 1e-2 and g["betas"] == (0.9, 0.999)
    assert g["eps"] == 1e-8 and g["lr"] == 1e-3
    for name, cls in (("sgd", FusedSGD), ("lars", LARS), ("adamw", AdamW)):
        args = build_parser().parse_args(["--optimizer", name, "--weight-decay", "0.5",
                                          "--adam-beta1", "0.8", "--adam-beta2", "0.9",
                                          "--adam-eps", "1e-5", "--clip-grad-norm", "2"])
        opt = optimizer_from_args(args, _model().parameters(), 0.01)
        assert type(opt) is cls and opt.param_groups[0]["weight_decay"] == 0.5 and opt.guarded
        if cls is AdamW:
            assert opt.param_groups[0]["betas"] == (0.8, 0.9) and opt.param_groups[0]["eps"] == 1e-5


@pytest.mark.parametrize("argv", [["--adam-beta1", "1.0"], ["--adam-beta2", "-0.1"],
                                  ["--adam-eps", "-1e-8"], ["--weight-decay", "-1"],
                                  ["--optimizer", "adam"]])
def test_cli_refuses_bad_values(argv, capsys):
    from ddp_amd.utils.cli import build_parser
    with pytest.raises(SystemExit):
        build_parser().parse_args(argv)
    capsys.readouterr()


def test_part1_trains_saves_and_resumes_with_the_same_t(tmp_path):
    """part1/main.py on the CPU with --optimizer adamw --accum-steps 2: 4 batches are 2 optimizer
    steps; --resume continues t; --metrics records carry the optimizer's name."""
    ck, ck2, metrics = (str(tmp_path / n) for n in ("a.pt", "b.pt", "m.jsonl"))
    base = [sys.executable, os.path.join(REPO, "part1", "main.py"), "--device", "cpu",
            "--train-size", "32", "--test-size", "8", "--global-batch", "4", "--threads", "2",
            "--optimizer", "adamw", "--lr", "0.001", "--accum-steps", "2", "--lr-schedule",
            "cosine", "--warmup-steps", "1", "--clip-grad-norm", "5", "--ema-decay", "0.9"]
    r = subprocess.run(base + ["--max-batches", "4", "--save", ck, "--metrics", metrics],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    sd = torch.load(ck, weights_only=True)["optimizer"]
    assert sd["lr_schedule"]["step"] == 2
    assert all(float(s["step"]) == 2.0 for s in sd["state"].values())
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    recs = [json.loads(ln) for ln in open(metrics)]
    iters = [rec for rec in recs if rec.get("event") == "iter"]
    assert iters and all(rec["optimizer"] == "adamw" for rec in iters)
    r = subprocess.run(base + ["--max-batches", "2", "--resume", ck, "--save", ck2],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    sd2 = torch.load(ck2, weights_only=True)["optimizer"]
    assert sd2["lr_schedule"]["step"] == 3
    assert not torch.equal(sd2["state"][0]["exp_avg_sq"], sd["state"][0]["exp_avg_sq"])


# --------------------------------------------------------------------------------- refusals
def test_updates_outside_the_launch_are_refused():
    from ddp_amd.optim import AdamW
    from ddp_amd.optim.arena import ParamArena
    from ddp_amd.parallel.zero import ShardedBf16Update, ShardedUpdate, arena_buckets

    class Comm:
        world, rank = 2, 0

    model = _model()
    arena = ParamArena(list(model.parameters()))
    opt = AdamW(model.parameters())
    assert opt.updates_in_launch_only is True and "AdamW" in opt.launch_only_reason
    buckets = arena_buckets(arena, [2])
    for cls in (ShardedUpdate, ShardedBf16Update):
        with pytest.raises(ValueError, match='AdamW.*update="allreduce"'):
            cls(arena, opt, Comm(), buckets)
    with pytest.raises(ValueError, match='AdamW.*update="allreduce"'):
        opt.step_elements(0, 64)
    with pytest.raises(RuntimeError, match="AdamW"):
        opt.register_in_backward()
    with pytest.raises(RuntimeError, match="AdamW"):
        opt.step(fused_taken=True)
    opt.set_ema(0.9)   # both reasons are named
    assert "AdamW" in opt.launch_only_reason and "EMA" in opt.launch_only_reason
    with pytest.raises(RuntimeError, match="EMA"):
        opt.register_in_backward()


def test_the_launch_refuses_lars_with_adam():
    """ddp_sgd_pack returns -1 for LarsArgs and AdamArgs together before it launches anything
    (the pointers are never read): the binding raises."""
    import __graft_entry__ as g
    g.build()
    import ddp_amd
    nat = ddp_amd.native()
    adam = dict(sched=64, adam_v=64, adam_bias=64, adam_n_bias=1, adam_omb1=0.1, adam_beta2=0.9,
                adam_omb2=0.1, adam_eps=1e-8)
    with pytest.raises(RuntimeError):
        nat.sgd_pack(64, 1, 64, 64, 64, 64, 0.1, 0.0, 0.0, 1.0, 0, 0, lars_side=64,
                     lars_tensors=64, lars_partial=64, lars_trust=64, **adam)
    with pytest.raises(TypeError):
        nat.sgd_pack(64, 1, 64, 64, 64, 64, 0.1, 0.0, 0.0, 1.0, 0, 0, adam_unknown=1)


def test_train_step_keeps_the_update_out_of_the_backward(monkeypatch):
    """TrainStep.opt_in_bwd with a stand-in fused optimizer and device loader that answers
    ``updates_in_launch_only`` as AdamW does."""
    from ddp_amd.engine import step as st
    from ddp_amd.optim import AdamW, FusedSGD

    class Loader:
        device = "cpu"

        def cursor_advance(self, m):
            return (0, m)

    def stand_in(real):
        class Opt:
            _fused = True
            updates_in_launch_only = real.updates_in_launch_only
            needs_whole_tensors = getattr(real, "needs_whole_tensors", False)

            def zero_grad(self):
                pass

            def register_in_backward(self):
                pass
        return Opt()

    for k in ("DDP_AMD_SGD_IN_BWD", "DDP_AMD_EMULATE_COMM", "DDP_AMD_EMULATE_COMM_GBPS"):
        monkeypatch.delenv(k, raising=False)
    model, crit = torch.nn.Linear(2, 2), torch.nn.CrossEntropyLoss()
    sgd = stand_in(FusedSGD(_model().parameters(), lr=0.1))
    adam = stand_in(AdamW(_model().parameters()))
    assert st.TrainStep(model, sgd, crit, Loader()).opt_in_bwd is True
    assert st.TrainStep(model, adam, crit, Loader()).opt_in_bwd is False


# ------------------------------------------------------------------------------------- Gloo
def test_gloo_ddp_replicas_are_identical_and_match_one_process():
    """World 2, 3 steps: the replicas end bit-identical, and equal to a single process on the
    concatenated batch within the tolerance of tests/test_dist_cpu.py's strategy comparison
    (rtol 1e-5, atol 1e-6)."""
    from adamw_dist_worker import batch, ddp_adamw_worker, model
    from dist_helpers import run_workers
    from ddp_amd.optim import AdamW
    steps, n = 3, 4
    out = run_workers(ddp_adamw_worker, 2, steps, n)
    for r, v in out.items():
        assert "error" not in v, v.get("error")
        assert v["consistent"] and v["t"] == steps and v["n_buckets"] > 1
    assert torch.equal(_bits(out[0]["params"]), _bits(out[1]["params"]))
    assert torch.equal(_bits(out[0]["v"]), _bits(out[1]["v"]))
    single = model()
    opt = AdamW(single.parameters(), lr=1e-3)
    for s in range(steps):
        xs, ys = zip(*(batch(s, r, n) for r in range(2)))
        opt.zero_grad()
        torch.nn.functional.cross_entropy(single(torch.cat(xs)), torch.cat(ys)).backward()
        opt.step()
    want = torch.cat([p.detach().reshape(-1) for p in single.parameters()])
    assert torch.allclose(out[0]["params"], want, rtol=1e-5, atol=1e-6)
    start = torch.cat([p.detach().reshape(-1) for p in model().parameters()])
    assert float((want - start).abs().max()) > 1e-4   # three steps of about lr each
