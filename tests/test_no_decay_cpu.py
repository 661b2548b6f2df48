"""The no-decay mask (``no_decay``, --no-decay-1d) on the CPU: the four optimizer classes against
torch's two param groups and the oracles, the mask's bookkeeping (param group, state dict,
tables), the command line, and the sharded updates on Gloo. The CPU classes are the oracles of
the GPU tests (tests/test_gpu_no_decay.py)."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import adamw_oracle as ao
import decay_oracle as do
import lamb_oracle as lo
from exactness import FP32_EPS, assert_within, int_tensor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WD = 0.05


def _model(seed=0):
    """As tests/test_adamw_cpu.py ``_model``: conv + BatchNorm + linear; parameters 1, 2, 3 and 5
    (conv bias, gamma, beta, linear bias) are 1-D."""
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 6, 3, padding=1), torch.nn.BatchNorm2d(6),
                               torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(6 * 8 * 8, 5))


ONE_D = [1, 2, 3, 5]


def _backward(model, step, scale=1.0):
    g = torch.Generator().manual_seed(100 + step)
    x, y = torch.randn(4, 3, 8, 8, generator=g), torch.randint(0, 5, (4,), generator=g)
    (scale * torch.nn.functional.cross_entropy(model(x), y)).backward()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _two_groups(model, wd):
    ps = list(model.parameters())
    return [{"params": [p for p in ps if p.dim() > 1], "weight_decay": wd},
            {"params": [p for p in ps if p.dim() <= 1], "weight_decay": 0.0}]


# ------------------------------------------------------------------------------- against torch
@pytest.mark.parametrize("nesterov", [False, True])
def test_sgd_is_torch_sgd_with_two_groups_bit_for_bit(nesterov):
    from ddp_amd.optim import FusedSGD
    model, twin = _model(), _model()
    opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=WD, nesterov=nesterov,
                   no_decay="1d")
    ref = torch.optim.SGD(_two_groups(twin, WD), lr=0.1, momentum=0.9, nesterov=nesterov)
    assert opt.no_decay_mask == [False, True, True, True, False, True]
    for k in range(3):
        for o, m in ((opt, model), (ref, twin)):
            o.zero_grad()
            _backward(m, k)
            o.step()
    for p, q in zip(model.parameters(), twin.parameters()):
        assert torch.equal(_bits(p), _bits(q))
        assert torch.equal(_bits(opt.state[p]["momentum_buffer"]),
                           _bits(ref.state[q]["momentum_buffer"]))
    # and the decay is really off the vectors: the unmasked twin differs there
    plain = _model()
    po = FusedSGD(plain.parameters(), lr=0.1, momentum=0.9, weight_decay=WD, nesterov=nesterov)
    for k in range(3):
        po.zero_grad()
        _backward(plain, k)
        po.step()
    assert not torch.equal(list(plain.parameters())[2], list(model.parameters())[2])


def test_adamw_against_torch_adamw_with_two_groups():
    """The tolerance of tests/test_adamw_cpu.py against torch.optim.AdamW (atol 1e-6 at this
    learning rate: |dp| <= about lr per step, fp32 roundings)."""
    from ddp_amd.optim import AdamW
    model, twin = _model(), _model()
    opt = AdamW(model.parameters(), lr=2e-3, weight_decay=WD, no_decay="1d")
    ref = torch.optim.AdamW(_two_groups(twin, WD), lr=2e-3)
    for k in range(3):
        for o, m in ((opt, model), (ref, twin)):
            o.zero_grad()
            _backward(m, k)
            o.step()
        with torch.no_grad():
            for p, q in zip(model.parameters(), twin.parameters()):
                assert torch.allclose(p, q, rtol=0, atol=1e-6), k
                # The conv bias in front of BatchNorm has a gradient of pure rounding noise
                # (1e-9), which Adam normalises to a step of order lr: one ulp of difference in
                # the weights would give it another direction in the next step. Every step is
                # compared from the same weights; the moments stay each optimizer's own.
                p.copy_(q)
    # an all-decayed twin is further away than that on gamma (|gamma| = 1: lr wd per step)
    full = _model()
    fo = AdamW(full.parameters(), lr=2e-3, weight_decay=WD)
    for k in range(3):
        fo.zero_grad()
        _backward(full, k)
        fo.step()
    assert not torch.allclose(list(full.parameters())[2], list(twin.parameters())[2], rtol=0,
                              atol=1e-5)


def test_adamw_is_bitwise_the_oracle_with_wd_zero_on_the_masked_tensors():
    from ddp_amd.optim import AdamW
    model = _model(1)
    ps = list(model.parameters())
    opt = AdamW(ps, lr=1e-3, weight_decay=WD, grad_scale=0.5, no_decay="1d")
    # the model's "1d" mask, one step from a fresh state: within the kernel's bound of the oracle
    # (tests/test_adamw_cpu.py test_cpu_path_is_within_the_kernels_bound_of_the_oracle)
    _backward(model, 0)
    a1, a2 = opt.bias_at(0)
    hp = ao.hyper(1e-3, WD, 0.5, 0.9, 0.999, 1e-8, a1, a2)
    before = [(p.detach().reshape(-1).clone(), p.grad.reshape(-1).clone()) for p in ps]
    opt.step()
    for i, p in enumerate(ps):
        p0, g0 = before[i]
        z, masked = torch.zeros_like(p0), torch.full((p0.numel(),), i in ONE_D)
        want = do.adamw_ref(p0, g0, z, z, hp, masked)
        bd = ao.bounds(do.adamw_abs(p0, g0, z, z, hp, masked), FP32_EPS)
        assert_within(p.detach().reshape(-1), want[0], bd["p"], what=f"parameter {i}")
        if i in ONE_D:   # and it is the wd = 0 rule: the decayed oracle is outside the bound
            other = ao.adamw_ref(p0, g0, z, z, hp)[0]
            far = (other - want[0]).abs() > 4 * bd["p"]
            assert bool(far.any()) or not bool(p0.any()), i
    # bitwise: a state whose every intermediate is an fp32 number (tests/test_gpu_adamw_exact.py)
    n = 4096 + 7
    g = int_tensor((n,), 1, 64, 3) * (2 * int_tensor((n,), 0, 1, 4) - 1)
    a = int_tensor((n,), 1, 3, 5) * (2 * int_tensor((n,), 0, 1, 6) - 1)
    b = 2.0 ** int_tensor((n,), 0, 2, 7)
    p0, gr, m0, v0 = 8 * int_tensor((n,), -4, 4, 8), 2 * g, (2 * a - 1) * g, (2 * b * b - 1) * g * g
    hp = dict(lr=2.0 ** -2, wd=2.0 ** -3, grad_scale=0.5, omb1=0.5, beta2=0.5, omb2=0.5, eps=0.0,
              a1=2.0, a2=0.5)
    q0, q1 = torch.nn.Parameter(p0.clone()), torch.nn.Parameter(p0.clone())
    opt = AdamW([q0, q1], lr=2.0 ** -2, betas=(0.5, 0.5), eps=0.0, weight_decay=2.0 ** -3,
                grad_scale=0.5, no_decay=[q1])
    opt._bias = np.array([[2.0, 0.5]], dtype=np.float32)
    for q in (q0, q1):
        opt.state[q] = {"step": torch.tensor(0.0), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
        q.grad = gr.clone()
    opt.step()
    for q, masked in ((q0, False), (q1, True)):
        w = do.adamw_ref(p0, gr, m0, v0, hp, torch.full((n,), masked), exact=True)
        st = opt.state[q]
        for name, got, x in (("p", q, w[0]), ("m", st["exp_avg"], w[1]), ("v", st["exp_avg_sq"], w[2])):
            assert torch.equal(_bits(got), _bits(x.float())), (masked, name)
    assert not torch.equal(q0, q1)


# ------------------------------------------------------------------------------ LARS and LAMB
def test_lars_masked_adapted_tensor_has_no_wd_term_in_its_ratio():
    """The definition in float64 (tests/test_lars_cpu.py: rel 1e-6 on the ratios)."""
    from ddp_amd.optim import LARS
    eta, eps = 0.02, 1e-8
    for mask in (None, "1d"):
        model = _model(2)
        ps = list(model.parameters())
        opt = LARS(ps, lr=0.1, momentum=0.9, weight_decay=WD, trust_coefficient=eta, eps=eps,
                   exclude_1d=False, no_decay=mask)
        _backward(model, 0)
        want, newp = [], []
        for i, p in enumerate(ps):
            wd = 0.0 if (mask and i in ONE_D) else WD
            p64, g64 = p.detach().double(), p.grad.double()
            wn, gn = float(p64.norm()), float(g64.norm())
            t = eta * wn / (gn + wd * wn + eps) if wn > 0 and gn > 0 else 1.0
            want.append(t)
            newp.append(p64 - 0.1 * t * (g64 + wd * p64))
        opt.step()
        got = opt.trust_ratios()
        for i, p in enumerate(ps):
            assert float(got[i]) == pytest.approx(want[i], rel=1e-6), (mask, i)
            torch.testing.assert_close(p.detach().double(), newp[i], rtol=1e-6, atol=1e-7)
    # the wd term matters at this decay: gamma's ratio with and without it are apart
    p = ps[2].detach().double()
    assert WD * float(p.norm()) > 1e-3 * float(ps[2].grad.double().norm())


def test_lamb_masked_adapted_tensor_forms_its_direction_without_wd():
    """The crafted exact state of tests/test_lamb_cpu.py: the CPU class returns the oracle's
    ratio, m, v and p' bit for bit, with wd = 0 for the masked tensor and wd for its neighbour."""
    from ddp_amd.optim import LAMB
    n = 8192 + 330
    g = int_tensor((n,), 1, 64, 1) * (2 * int_tensor((n,), 0, 1, 2) - 1)
    a = int_tensor((n,), 1, 3, 3) * (2 * int_tensor((n,), 0, 1, 4) - 1)
    b = 2.0 ** int_tensor((n,), 0, 2, 5)
    p0, gr, m0, v0 = 8 * int_tensor((n,), -4, 4, 6), 2 * g, (2 * a - 1) * g, (2 * b * b - 1) * g * g
    hp = dict(lr=2.0 ** -2, wd=2.0 ** -3, grad_scale=0.5, omb1=0.5, beta2=0.5, omb2=0.5, eps=0.0,
              a1=2.0, a2=0.5)
    q0, q1 = torch.nn.Parameter(p0.clone()), torch.nn.Parameter(p0.clone())
    opt = LAMB([q0, q1], lr=2.0 ** -2, betas=(0.5, 0.5), eps=0.0, weight_decay=2.0 ** -3,
               grad_scale=0.5, exclude_1d=False, no_decay="1d")
    opt.set_no_decay([q1])
    assert opt.no_decay_mask == [False, True]
    opt._bias = np.array([[2.0, 0.5]], dtype=np.float32)
    for q in (q0, q1):
        opt.state[q] = {"step": torch.tensor(0.0), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
        q.grad = gr.clone()
    opt.step()
    ratios = []
    for i, (q, masked) in enumerate(((q0, False), (q1, True))):
        h = dict(hp, wd=0.0) if masked else hp
        r, nm, nv = lo.direction(p0, gr, m0, v0, h, exact=True)
        sp, sr = lo.sum_sq(p0, exact=True), lo.sum_sq(r, exact=True)
        trust = float(np.float32(np.float32(np.sqrt(sp)) / np.float32(np.sqrt(sr))))
        want = do.lamb_ref(p0, gr, m0, v0, hp, masked, trust=trust)[0]
        assert float(opt.trust_ratios()[i]) == trust != 1.0
        assert torch.equal(_bits(q), _bits(want.float())), masked
        assert torch.equal(_bits(opt.state[q]["exp_avg_sq"]), _bits(nv.float()))
        ratios.append(trust)
    assert ratios[0] != ratios[1]   # the unmasked ratio has the wd term, the masked one has not


# ------------------------------------------------------------------------------ mask handling
def test_none_changes_nothing_in_groups_and_state_dict():
    from ddp_amd.optim import AdamW, FusedSGD, LAMB, LARS
    for cls, ref in ((FusedSGD, torch.optim.SGD), (LARS, None), (AdamW, None), (LAMB, None)):
        model = _model()
        opt = cls(model.parameters(), lr=0.01, weight_decay=WD, no_decay=None)
        assert "no_decay" not in opt.param_groups[0] and "no_decay" not in opt.defaults
        assert "no_decay" not in opt.state_dict()["param_groups"][0]
        assert opt.no_decay_mask == [False] * 6 and opt.no_decay_name is None
        if ref is not None:
            rd = ref(_model().parameters(), lr=0.01, weight_decay=WD).state_dict()
            assert set(opt.state_dict()["param_groups"][0]) == set(rd["param_groups"][0])
    opt = FusedSGD(_model().parameters(), lr=0.01, no_decay="1d")
    opt.set_no_decay(None)
    assert "no_decay" not in opt.param_groups[0] and not any(opt.no_decay_mask)


@pytest.mark.parametrize("name", ["sgd", "lars", "adamw", "lamb"])
def test_mask_round_trips_through_a_weights_only_checkpoint(tmp_path, name):
    from ddp_amd.optim import AdamW, FusedSGD, LAMB, LARS
    cls = dict(sgd=FusedSGD, lars=LARS, adamw=AdamW, lamb=LAMB)[name]
    model = _model()
    opt = cls(model.parameters(), lr=0.01, weight_decay=WD, no_decay="1d")
    _backward(model, 0)
    opt.step()
    sd = opt.state_dict()
    assert sd["param_groups"][0]["no_decay"] == ONE_D
    assert all(type(i) is int for i in sd["param_groups"][0]["no_decay"])
    f = str(tmp_path / "o.pt")
    torch.save(sd, f)
    other = cls(_model().parameters(), lr=0.01, weight_decay=WD)
    assert not any(other.no_decay_mask)
    other.load_state_dict(torch.load(f, weights_only=True))
    assert other.no_decay_mask == opt.no_decay_mask and other.no_decay_name == "1d"
    assert other.param_groups[0]["no_decay"] == ONE_D


def test_a_torch_state_dict_leaves_the_mask_alone():
    from ddp_amd.optim import AdamW, FusedSGD
    for cls, tcls, kw in ((FusedSGD, torch.optim.SGD, dict(momentum=0.9)),
                          (AdamW, torch.optim.AdamW, {})):
        src = _model()
        topt = tcls(src.parameters(), lr=0.01, weight_decay=WD, **kw)
        _backward(src, 0)
        topt.step()
        for mask in (None, "1d"):
            opt = cls(_model().parameters(), lr=0.01, weight_decay=WD, no_decay=mask, **kw)
            opt.load_state_dict(copy.deepcopy(topt.state_dict()))
            assert opt.no_decay_mask == [mask is not None and i in ONE_D for i in range(6)]
            assert ("no_decay" in opt.param_groups[0]) == (mask is not None)


def test_iterable_form_and_unknown_tensor():
    from ddp_amd.optim import FusedSGD
    model = _model()
    ps = list(model.parameters())
    opt = FusedSGD(ps, lr=0.1, weight_decay=WD, no_decay=[ps[4], ps[2]])
    assert opt.no_decay_mask == [False, False, True, False, True, False]
    assert opt.param_groups[0]["no_decay"] == [2, 4] and opt.no_decay_name == "custom"
    with pytest.raises(ValueError):
        opt.set_no_decay([torch.nn.Parameter(torch.zeros(6))])   # equal shape, another tensor
    with pytest.raises(ValueError):
        FusedSGD(_model().parameters(), lr=0.1, no_decay="2d")
    assert opt.no_decay_mask == [False, False, True, False, True, False]
    # matched by identity, not by value
    twin = _model()
    with pytest.raises(ValueError):
        opt.set_no_decay([list(twin.parameters())[2]])


def test_element_runs_follow_the_mask_and_the_padding():
    """``_decay_runs`` / ``_elem_table``'s cut: padding goes with the tensor before it, equal
    neighbours merge; the CPU ``step_elements`` applies wd per run."""
    from ddp_amd.optim import FusedSGD
    from ddp_amd.optim.arena import ParamArena
    model = _model()
    ps = list(model.parameters())
    a = ParamArena(ps, krsc=False)
    opt = FusedSGD(ps, lr=0.5, weight_decay=0.25, no_decay="1d")
    assert opt.arena is a
    o = a.offsets
    assert opt._decay_runs(0, a.total) == [(0, o[1], False), (o[1], o[4], True),
                                           (o[4], o[5], False), (o[5], a.total, True)]
    assert opt._decay_runs(o[1] - 3, o[1] + 2) == [(o[1] - 3, o[1], False), (o[1], o[1] + 2, True)]
    plain = FusedSGD(ps, lr=0.5, weight_decay=0.25)
    assert plain._decay_runs(5, 77) == [(5, 77, False)]
    with torch.no_grad():
        a.data.fill_(1.0)
        a.grad.fill_(2.0)
    lo_, hi_ = o[1] - 3, o[1] + 2
    opt.step_elements(lo_, hi_)
    want = torch.ones(a.total)
    want[lo_:o[1]] = 1.0 - 0.5 * (2.0 + 0.25)
    want[o[1]:hi_] = 1.0 - 0.5 * 2.0
    assert torch.equal(a.data, want)


# ------------------------------------------------------------------------------- command line
def test_cli_flag_and_optimizer_from_args():
    from ddp_amd.optim import AdamW, FusedSGD, LAMB, LARS
    from ddp_amd.utils.cli import build_parser, optimizer_from_args
    assert build_parser().parse_args([]).no_decay_1d is False
    for name, cls in (("sgd", FusedSGD), ("lars", LARS), ("adamw", AdamW), ("lamb", LAMB)):
        args = build_parser().parse_args(["--optimizer", name, "--no-decay-1d"])
        assert args.no_decay_1d is True
        opt = optimizer_from_args(args, _model().parameters(), 0.01)
        assert type(opt) is cls and opt.no_decay_mask == [i in ONE_D for i in range(6)]
        off = optimizer_from_args(build_parser().parse_args(["--optimizer", name]),
                                  _model().parameters(), 0.01)
        assert not any(off.no_decay_mask) and "no_decay" not in off.param_groups[0]


def test_part1_records_the_field_and_the_checkpoint_keeps_the_mask(tmp_path):
    ck, ck2, metrics, m2 = (str(tmp_path / n) for n in ("a.pt", "b.pt", "m.jsonl", "n.jsonl"))
    base = [sys.executable, os.path.join(REPO, "part1", "main.py"), "--device", "cpu",
            "--train-size", "16", "--test-size", "8", "--global-batch", "4", "--threads", "2",
            "--max-batches", "3", "--no-test"]
    r = subprocess.run(base + ["--no-decay-1d", "--save", ck, "--metrics", metrics],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    iters = [rec for rec in map(json.loads, open(metrics)) if rec.get("event") == "iter"]
    assert iters and all(rec["no_decay"] == "1d" for rec in iters)
    mask = torch.load(ck, weights_only=True)["optimizer"]["param_groups"][0]["no_decay"]
    assert mask and all(type(i) is int for i in mask)
    # resumed WITHOUT the flag: the checkpoint carries the mask
    r = subprocess.run(base + ["--resume", ck, "--save", ck2, "--metrics", m2],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert torch.load(ck2, weights_only=True)["optimizer"]["param_groups"][0]["no_decay"] == mask
    iters = [rec for rec in map(json.loads, open(m2)) if rec.get("event") == "iter"]
    assert iters and all(rec["no_decay"] == "1d" for rec in iters)


# ------------------------------------------------------------------------------ Gloo, world 2
@pytest.mark.parametrize("mode", ["zero", "shard16"])
def test_sharded_updates_equal_their_replicated_masked_twins(mode):
    """ShardedUpdate / ShardedBf16Update with the mask at world 2, three steps: bit-identical to
    the replicated masked update, replicas bit-identical; the last bucket's shard boundary lies
    inside the classifier's weight, so rank 0's shard holds masked runs (the last BatchNorm's
    gamma and beta) and an unmasked one, rank 1's an unmasked one and the masked bias."""
    from dist_helpers import run_workers
    from no_decay_dist_worker import sharded_worker
    out = run_workers(sharded_worker, 2, mode, 3)
    for r, v in out.items():
        assert "error" not in v, v.get("error")
        assert v["grad_zero"] and v["consistent"] and v["mixed_shards"] == [True, True]
    assert torch.equal(_bits(out[0]["sharded"]), _bits(out[1]["sharded"]))
    assert torch.equal(_bits(out[0]["sharded"]), _bits(out[0]["replicated"]))
    assert torch.equal(_bits(out[0]["sharded_momentum"]), _bits(out[0]["replicated_momentum"]))
    # the mask did something: the all-decayed replicated twin differs on the masked elements only
    # by more than rounding after three steps at this decay
    assert not torch.equal(out[0]["replicated"], out[0]["replicated_all_decayed"])
