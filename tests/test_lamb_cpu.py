"""LAMB on the CPU (optim/lamb.py, utils/cli.py, mains, checkpoints): the CPU class is the oracle
of the LAMB kernels and the optimizer of the Gloo paths. The rule and its oracle:
tests/lamb_oracle.py."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import adamw_oracle as ao
import lamb_oracle as lo
import test_adamw_cpu as ta
from exactness import FP32_EPS, assert_within, int_tensor

REPO = ta.REPO
_model, _backward, _bits = ta._model, ta._backward, ta._bits


def _lamb(params, **kw):
    from ddp_amd.optim import LAMB
    return LAMB(params, **kw)


def _history(opt, ps, seed, t):
    """A non-zero m and v history and the step word of step ``t``."""
    gen = torch.Generator().manual_seed(seed)
    for p in ps:
        opt.state[p] = {"step": torch.tensor(float(t - 1)),
                        "exp_avg": 0.1 * torch.randn(p.shape, generator=gen),
                        "exp_avg_sq": 0.02 * torch.rand(p.shape, generator=gen) + 1e-6}
    opt.set_lr_step(t - 1)


# ------------------------------------------------------------------------------------ the rule
def test_cpu_class_against_textbook_lamb():
    """One step at t = 3 from a history in m and v, against LAMB as the paper writes it (You et
    al. 2020, Algorithm 2 with phi = identity), in fp64 on the same fp32 inputs:
        m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  mh = m / (1 - b1^t);  vh = v / (1 - b2^t)
        r = mh / (sqrt(vh) + eps) + wd p;   p -= lr (|p| / |r|) r    (2-D tensors; 1-D: ratio 1)
    Hyper-parameters that are fp32 numbers (lr 2**-10, betas (1 - 2**-3, 1 - 2**-8), eps 2**-27,
    wd 2**-7), so both sides get the same values.

    The bound, first order in eps = 2**-24, every count an integer number of roundings. With
    T_m, T_u, den of tests/test_adamw_cpu.py test_cpu_path_against_real_arithmetic and
    T_r = wd |p| + a1 T_u:
      u   = fl(m' / den)              9 eps T_u          (8, + 1 for the table's rounding of a2)
      a1 u                            (9 + 1 for the table's a1 + 1) = 11 eps a1 T_u
      r   = fma(wd, p, a1 u)          11 eps a1 T_u + eps T_r <= 12 eps T_r              =: E_r
      sum p^2: fp64, rounded once     1 eps relative;  wn = sqrt: 1/2 + 1
      sum r^2: |sum fl(r)^2 - sum r^2| <= 2 sum |r| E_r = 24 eps A sum r^2,
               A = sum(|r| T_r) / sum r^2; rounded once: + 1;  rn = sqrt: (24 A + 1) / 2 + 1
      trust = fl(wn / rn)             (3/2 + 12 A + 3/2 + 1) = (4 + 12 A) eps relative
      lt  = fl(lr trust)              (5 + 12 A) eps relative
      p'  = fma(-lt, r, p)            lt |r| (5 + 12 A) eps + lt E_r + eps (|p| + lt |r|)
                                   <= eps (|p| + lt (12 T_r + (6 + 12 A) |r|))
    A tensor with ratio 1 has no error in the ratio: eps (|p| + lt (12 T_r + |r|)).
    Magnitudes are taken from the fp64 run."""
    lr, b1, b2, eps, wd, t = 2.0 ** -10, 1 - 2.0 ** -3, 1 - 2.0 ** -8, 2.0 ** -27, 2.0 ** -7, 3
    model = _model(3)
    ps = list(model.parameters())
    opt = _lamb(ps, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    _history(opt, ps, 21, t)
    _backward(model, 1)
    a1, a2 = opt.bias_at(t - 1)
    hp = ao.hyper(lr, wd, 1.0, b1, b2, eps, a1, a2)
    want, bound, ratios = [], [], []
    for p in ps:
        st = opt.state[p]
        p64, g64 = p.detach().double(), p.grad.double()
        m = b1 * st["exp_avg"].double() + (1 - b1) * g64
        v = b2 * st["exp_avg_sq"].double() + (1 - b2) * g64 * g64
        r = (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps) + wd * p64
        ratio = float(p64.norm() / r.norm()) if p.dim() > 1 else 1.0
        T = lo.lamb_abs(p64, g64, st["exp_avg"], st["exp_avg_sq"], hp)
        A = float((r.abs() * T["T_r"]).sum() / (r * r).sum())
        lt = lr * ratio
        extra = (6 + 12 * A) if p.dim() > 1 else 1
        want.append(p64 - lt * r)
        bound.append(FP32_EPS * (T["p"] + lt * (12 * T["T_r"] + extra * r.abs())) + 16 * lo.TINY)
        ratios.append((ratio, (4 + 12 * A) * FP32_EPS))
    opt.step()
    worst = 0.0
    for i, p in enumerate(ps):
        worst = max(worst, assert_within(p.detach(), want[i], bound[i], what=f"parameter {i}"))
    print("worst |err| / bound:", worst, "ratios:", ratios)
    assert worst > 0.0 and opt.lr_step == t
    got = opt.trust_ratios()
    for i, p in enumerate(ps):
        assert (float(got[i]) == 1.0) == (p.dim() == 1)
        assert abs(float(got[i]) - ratios[i][0]) <= ratios[i][1] * ratios[i][0]
    assert any(abs(x - 1.0) > 0.1 for x, _ in ratios)


def _crafted(n, seed):
    """The exact-mode state of tests/test_gpu_adamw_exact.py with p in multiples of 8."""
    g = int_tensor((n,), 1, 64, seed) * (2 * int_tensor((n,), 0, 1, seed + 1) - 1)
    a = int_tensor((n,), 1, 3, seed + 2) * (2 * int_tensor((n,), 0, 1, seed + 3) - 1)
    b = 2.0 ** int_tensor((n,), 0, 2, seed + 4)
    p = 8 * int_tensor((n,), -4, 4, seed + 5)
    return p, 2 * g, (2 * a - 1) * g, (2 * b * b - 1) * g * g


EXACT_HP = dict(lr=2.0 ** -2, wd=2.0 ** -3, grad_scale=0.5, omb1=0.5, beta2=0.5, omb2=0.5, eps=0.0,
                a1=2.0, a2=0.5)


def test_crafted_state_is_exact_and_the_cpu_path_returns_it():
    """8192 + 330 elements of the crafted state: the oracle asserts that r is an integer and
    that no sum rounds in any order; the CPU class returns the oracle's m, v and ratio bit for
    bit, and p' with the one rounding of its last fma (the fp64 value behind it is exact: an
    integer minus a 24-bit ratio times an integer below 2^5)."""
    n = 8192 + 330
    p0, g, m0, v0 = _crafted(n, 1)
    r, nm, nv = lo.direction(p0, g, m0, v0, EXACT_HP, exact=True)
    assert bool((r == r.round()).all()) and float(r.abs().max()) <= 16
    sp, sr = lo.sum_sq(p0, exact=True), lo.sum_sq(r, exact=True)
    # fp32 sqrt and / of fp32 numbers, through fp64: 53 >= 2 * 24 + 2 bits, no double rounding
    trust = float(np.float32(np.float32(np.sqrt(sp)) / np.float32(np.sqrt(sr))))
    want = lo.apply(p0, r, EXACT_HP, trust)
    p = torch.nn.Parameter(p0.clone())
    opt = _lamb([p], lr=2.0 ** -2, betas=(0.5, 0.5), eps=0.0, weight_decay=2.0 ** -3,
                grad_scale=0.5, exclude_1d=False)
    opt._bias = np.array([[2.0, 0.5]], dtype=np.float32)   # the test's own table
    opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    p.grad = g.clone()
    opt.step()
    st = opt.state[p]
    assert float(opt.trust_ratios()[0]) == trust != 1.0
    for name, got, w in (("p", p, want), ("m", st["exp_avg"], nm), ("v", st["exp_avg_sq"], nv)):
        assert torch.equal(_bits(got), _bits(w.float())), name


def test_exclude_1d_false_adapts_vectors():
    for ex in (True, False):
        model = _model(4)
        opt = _lamb(model.parameters(), exclude_1d=ex)
        _backward(model, 0)
        zero = [not bool(p.any()) for p in model.parameters()]   # BatchNorm's beta: wn = 0
        assert sum(zero) == 1
        opt.step()
        for p, z, t in zip(model.parameters(), zero, opt.trust_ratios().tolist()):
            assert (t == 1.0) == ((p.dim() == 1 and ex) or z), (ex, tuple(p.shape), t)


def test_zero_norms_give_trust_one():
    """A zero gradient on zero moments with wd = 0: r = 0, rn = 0. A zero weight tensor: wn = 0."""
    w = torch.nn.Parameter(torch.randn(4, 5, generator=torch.Generator().manual_seed(1)))
    z = torch.nn.Parameter(torch.zeros(3, 4))
    opt = _lamb([w, z], weight_decay=0.0)
    w.grad, z.grad = torch.zeros_like(w), torch.ones_like(z)
    before = w.detach().clone()
    opt.step()
    assert opt.trust_ratios().tolist() == [1.0, 1.0]
    assert torch.equal(w, before)
    assert bool((z != 0).all())   # the step was taken at ratio 1: about -lr


# -------------------------------------------------------------------------------- the step number
def test_a_skipped_step_advances_t_and_leaves_the_state():
    model = _model()
    opt = _lamb(model.parameters(), skip_nonfinite=True)
    opt.set_ema(0.9)
    _backward(model, 0)
    opt.step()
    assert opt.lr_step == 1 and int(opt.skipped_steps()) == 0
    before = [p.detach().clone() for p in model.parameters()]
    state = [{k: v.clone() for k, v in opt.state[p].items()} for p in model.parameters()]
    ema, ratios = opt.ema.clone(), opt.trust_ratios().clone()
    assert bool((ratios != 1.0).any())
    opt.zero_grad()
    _backward(model, 1)
    next(model.parameters()).grad[0, 0, 0, 0] = float("inf")
    opt.step(zero_grad=True)
    assert opt.lr_step == 2 and int(opt.skipped_steps()) == 1
    for p, b, s in zip(model.parameters(), before, state):
        assert torch.equal(p, b) and not bool(p.grad.any())
        assert torch.equal(opt.state[p]["exp_avg"], s["exp_avg"])
        assert torch.equal(opt.state[p]["exp_avg_sq"], s["exp_avg_sq"])
    assert torch.equal(opt.ema, ema) and torch.equal(opt.trust_ratios(), ratios)


def test_an_accumulated_step_advances_t_once():
    """Two backward passes, one step at grad_scale 1/2 (what --accum-steps 2 does): one advance
    and one ratio, that of the mean gradient (a twin that is handed the mean directly)."""
    from ddp_amd.engine.trainer import grad_scaled
    model, twin = _model(), _model()
    opt, topt = _lamb(model.parameters()), _lamb(twin.parameters())
    for j in range(2):
        _backward(model, j)
        _backward(twin, j, scale=0.5)
    with grad_scaled(opt, 2):
        opt.step()
    topt.step()
    assert opt.lr_step == 1 == topt.lr_step
    assert torch.allclose(opt.trust_ratios(), topt.trust_ratios(), rtol=1e-5, atol=0)
    for p, q in zip(model.parameters(), twin.parameters()):
        # |dp| = lr trust |r|, r of order 1, trust below 10 here: fp32 roundings of the gradient sum
        assert torch.allclose(p, q, rtol=0, atol=2e-5)


# ------------------------------------------------------------------------------- checkpoints
def test_state_dict_round_trip_and_a_torch_adamw_state_dict_loads():
    from ddp_amd.optim import LAMB
    model = _model()
    opt = _lamb(model.parameters(), betas=(0.8, 0.99), exclude_1d=False, max_grad_norm=5.0)
    for k in range(2):
        opt.zero_grad()
        _backward(model, k)
        opt.step()
    sd = copy.deepcopy(opt.state_dict())   # (torch hands out, and takes in, its own tensors)
    g = sd["param_groups"][0]
    assert g["exclude_1d"] is False and tuple(g["betas"]) == (0.8, 0.99)
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    twin = _model()
    twin.load_state_dict(model.state_dict())
    other = LAMB(twin.parameters())
    other.load_state_dict(sd)
    assert other.lr_step == 2 and other.param_groups[0]["exclude_1d"] is False and other.guarded
    for o, m in ((opt, model), (other, twin)):
        o.zero_grad()
        _backward(m, 5)
        o.step()
    for p, q in zip(model.parameters(), twin.parameters()):
        assert torch.equal(_bits(p), _bits(q))
    assert torch.equal(opt.trust_ratios(), other.trust_ratios())
    # torch.optim.AdamW's state dict: no exclude_1d in its group, the constructor's stays
    ref = _model()
    topt = torch.optim.AdamW(ref.parameters(), lr=2e-3, betas=(0.85, 0.98))
    for k in range(3):
        topt.zero_grad()
        _backward(ref, k)
        topt.step()
    third = LAMB(_model().parameters())
    third.load_state_dict(copy.deepcopy(topt.state_dict()))
    g = third.param_groups[0]
    assert third.lr_step == 3 and tuple(g["betas"]) == (0.85, 0.98) and g["exclude_1d"] is True


def test_part1_trains_saves_and_resumes_with_the_same_t(tmp_path):
    ck, ck2, metrics = (str(tmp_path / n) for n in ("a.pt", "b.pt", "m.jsonl"))
    base = [sys.executable, os.path.join(REPO, "part1", "main.py"), "--device", "cpu",
            "--train-size", "32", "--test-size", "8", "--global-batch", "4", "--threads", "2",
            "--optimizer", "lamb", "--lr", "0.002", "--lr-schedule", "cosine", "--warmup-steps",
            "1", "--clip-grad-norm", "5", "--ema-decay", "0.9"]
    r = subprocess.run(base + ["--max-batches", "3", "--save", ck, "--metrics", metrics],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    sd = torch.load(ck, weights_only=True)["optimizer"]
    assert sd["lr_schedule"]["step"] == 3 and sd["param_groups"][0]["exclude_1d"] is True
    assert all(float(s["step"]) == 3.0 for s in sd["state"].values())
    iters = [rec for rec in map(json.loads, open(metrics)) if rec.get("event") == "iter"]
    assert iters and all(rec["optimizer"] == "lamb" for rec in iters)
    r = subprocess.run(base + ["--max-batches", "1", "--resume", ck, "--save", ck2],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert torch.load(ck2, weights_only=True)["optimizer"]["lr_schedule"]["step"] == 4


# --------------------------------------------------------------------------------------- CLI
def test_cli_builds_lamb_with_adamws_defaults():
    from ddp_amd.optim import LAMB
    from ddp_amd.utils.cli import build_parser, optimizer_from_args
    args = build_parser().parse_args(["--optimizer", "lamb", "--lr", "0.002"])
    opt = optimizer_from_args(args, _model().parameters(), args.lr)
    g = opt.param_groups[0]
    assert type(opt) is LAMB and g["weight_decay"] == 1e-2 and g["betas"] == (0.9, 0.999)
    assert g["eps"] == 1e-8 and g["lr"] == 2e-3 and g["exclude_1d"] is True
    assert opt.metrics_name == "lamb" and opt.needs_whole_tensors is True
    args = build_parser().parse_args(["--optimizer", "lamb", "--weight-decay", "0.5",
                                      "--adam-beta1", "0.8", "--adam-beta2", "0.9", "--adam-eps",
                                      "1e-5", "--clip-grad-norm", "2"])
    opt = optimizer_from_args(args, _model().parameters(), 0.01)
    g = opt.param_groups[0]
    assert type(opt) is LAMB and g["weight_decay"] == 0.5 and opt.guarded
    assert g["betas"] == (0.8, 0.9) and g["eps"] == 1e-5


# --------------------------------------------------------------------------------- refusals
def test_updates_outside_the_launch_are_refused():
    from ddp_amd.optim.arena import ParamArena
    from ddp_amd.parallel.zero import ShardedBf16Update, ShardedUpdate, arena_buckets

    class Comm:
        world, rank = 2, 0

    model = _model()
    arena = ParamArena(list(model.parameters()))
    opt = _lamb(model.parameters())
    assert opt.updates_in_launch_only is True and "LAMB" in opt.launch_only_reason
    buckets = arena_buckets(arena, [2])
    for cls in (ShardedUpdate, ShardedBf16Update):
        with pytest.raises(ValueError, match='LAMB.*update="allreduce"'):
            cls(arena, opt, Comm(), buckets)
    with pytest.raises(ValueError, match='LAMB.*update="allreduce"'):
        opt.step_elements(0, 64)
    with pytest.raises(RuntimeError, match="LAMB"):
        opt.register_in_backward()
    with pytest.raises(RuntimeError, match="LAMB"):
        opt.step(fused_taken=True)


def test_the_launch_refuses_lamb_without_adam_and_with_lars():
    """ddp_sgd_pack returns -1 before it launches anything (the pointers are never read)."""
    import __graft_entry__ as g
    g.build()
    import ddp_amd
    nat = ddp_amd.native()
    adam = dict(sched=64, adam_v=64, adam_bias=64, adam_n_bias=1, adam_omb1=0.1, adam_beta2=0.9,
                adam_omb2=0.1, adam_eps=1e-8)
    lamb = dict(lamb_side=64, lamb_tensors=64, lamb_partial=64, lamb_trust=64)
    lars = dict(lars_side=64, lars_tensors=64, lars_partial=64, lars_trust=64)
    base = (64, 1, 64, 64, 64, 64, 0.1, 0.0, 0.0, 1.0, 0, 0)
    for bad in (lamb, dict(adam, **lamb, **lars), dict(lamb, **lars),
                dict(adam, **dict(lamb, lamb_tensors=0)), dict(adam, **dict(lamb, lamb_partial=0)),
                dict(adam, **dict(lamb, lamb_trust=0))):
        with pytest.raises(RuntimeError):
            nat.sgd_pack(*base, **bad)
    with pytest.raises(RuntimeError):   # the norms launch without a bias table
        nat.lamb_norms(64, 1, 64, 64, 64, 0.0, 1.0, 64, 0, sched=64, adam_v=64)


# ------------------------------------------------------------------------------------- Gloo
@pytest.mark.parametrize("strategy", ["ddp", "gather_scatter", "allreduce"])
def test_gloo_replicas_are_identical_and_match_one_process(strategy):
    """World 2, 3 steps under DDP, 2A and 2B: the replicas end bit-identical, with the same
    ratios, and equal to a single process on the concatenated batch within the tolerance of
    tests/test_dist_cpu.py's strategy comparison (rtol 1e-5, atol 1e-6)."""
    from dist_helpers import run_workers
    from lamb_dist_worker import batch, lamb_worker, model
    steps, n = 3, 4
    out = run_workers(lamb_worker, 2, strategy, steps, n)
    for r, v in out.items():
        assert "error" not in v, v.get("error")
        assert v["t"] == steps
        if strategy == "ddp":
            assert v["consistent"] and v["n_buckets"] > 1
    assert torch.equal(_bits(out[0]["params"]), _bits(out[1]["params"]))
    assert torch.equal(_bits(out[0]["trust"]), _bits(out[1]["trust"]))
    single = model()
    opt = _lamb(single.parameters(), lr=2e-3)
    for s in range(steps):
        xs, ys = zip(*(batch(s, r, n) for r in range(2)))
        opt.zero_grad()
        torch.nn.functional.cross_entropy(single(torch.cat(xs)), torch.cat(ys)).backward()
        opt.step()
    want = torch.cat([p.detach().reshape(-1) for p in single.parameters()])
    assert torch.allclose(out[0]["params"], want, rtol=1e-5, atol=1e-6)
    assert torch.allclose(out[0]["trust"], opt.trust_ratios(), rtol=1e-4, atol=0)
    start = torch.cat([p.detach().reshape(-1) for p in model().parameters()])
    assert float((want - start).abs().max()) > 1e-4
