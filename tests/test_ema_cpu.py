"""Weight EMA on the CPU (optim/sgd.py set_ema, optim/lars.py, engine, mains, checkpoints): the
CPU classes are the oracle of the update kernel's EMA instantiations and the optimizers of the
Gloo paths.

    e = fma(float32(1 - decay), p_new - e, e)        once per optimizer step that was taken

Closed form: the recurrence over the weights snapshotted after each step, in fp32 (bit for bit)
and in fp64. fp32 against fp64: each step rounds twice (the subtraction, the fma), each rounding
errs by at most 2**-24 of a value bounded by max(|e|, |p|) -- e stays between its own start and
the weights, and |p - e| <= 2 max(|e|, |p|) is multiplied by 1 - decay <= 1/2 before it counts
(decay >= 0.5 here; the difference itself is the quantity rounded, at half the weight) -- and the
errors of earlier steps are carried with weight decay < 1: 2 * T * 2**-24 * max(|e|, |p|)."""
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOM, WD = 0.9, 1e-4


def _model(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 6, 3, padding=1), torch.nn.BatchNorm2d(6),
                               torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(6 * 8 * 8, 5))


def _batch(step, n=4):
    g = torch.Generator().manual_seed(100 + step)
    return torch.randn(n, 3, 8, 8, generator=g), torch.randint(0, 5, (n,), generator=g)


def _backward(model, step):
    x, y = _batch(step)
    torch.nn.functional.cross_entropy(model(x), y).backward()


def _weights(model):
    return [p.detach().clone() for p in model.parameters()]


def _recurrence(snaps, decay, dtype=torch.float32):
    """The lerp recurrence over ``snaps`` = [start, after step 1, ...] per parameter."""
    from ddp_amd.optim.sgd import ema_lerp, one_minus_decay
    omd = one_minus_decay(decay)
    e = [w.to(dtype).clone() for w in snaps[0]]
    for snap in snaps[1:]:
        if dtype == torch.float32:
            e = [ema_lerp(ei, p, omd) for ei, p in zip(e, snap)]
        else:
            e = [ei + omd * (p.double() - ei) for ei, p in zip(e, snap)]
    return e


def _check_closed_form(cls, decay, T, **kw):
    model = _model()
    opt = cls(model.parameters(), lr=0.05, momentum=MOM, weight_decay=WD, **kw)
    assert opt.ema is None and opt.ema_decay is None and opt.updates_in_launch_only is False
    opt.set_ema(decay)
    assert opt.ema_decay == decay and opt.updates_in_launch_only is True
    assert opt.ema.dtype == torch.float32 and opt.ema.dim() == 1
    snaps = [_weights(model)]
    for step in range(T):
        opt.zero_grad()
        _backward(model, step)
        opt.step()
        snaps.append(_weights(model))
    got = list(opt.ema_state().values())
    want32, want64 = _recurrence(snaps, decay), _recurrence(snaps, decay, torch.float64)
    moved = False
    for i, (g, w32, w64) in enumerate(zip(got, want32, want64)):
        assert torch.equal(g, w32), i
        big = torch.stack([s[i].double().abs() for s in snaps] + [w64.abs()]).amax(0)
        err = (g.double() - w64).abs()
        worst = float((err / (2 * T * 2.0 ** -24 * big).clamp_min(1e-300)).max())
        print(f"parameter {i}: worst |fp32 - fp64| / bound {worst:.3f}")
        assert bool((err <= 2 * T * 2.0 ** -24 * big).all()), (i, worst)
        moved |= not torch.equal(g, snaps[0][i])
    assert moved
    return opt, model


def test_closed_form():
    from ddp_amd.optim import FusedSGD
    _check_closed_form(FusedSGD, 0.9, 5)


def test_closed_form_lars():
    from ddp_amd.optim import LARS
    _check_closed_form(LARS, 0.9, 5, trust_coefficient=0.02)


def test_lerp_form_keeps_equal_values_to_the_bit():
    """decay 0.5, p held constant and equal to e: the lerp form returns e itself (the sum form
    decay * e + (1 - decay) * p would round)."""
    from ddp_amd.optim import FusedSGD
    g = torch.Generator().manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(1000, generator=g) * 10.0 ** torch.randint(
        -20, 20, (1000,), generator=g).float())]
    opt = FusedSGD(ps, lr=0.0, momentum=0.0, weight_decay=0.0)
    opt.set_ema(0.5)
    start = ps[0].detach().clone()
    for _ in range(3):
        ps[0].grad = torch.ones(1000)
        opt.step()
    assert torch.equal(ps[0].detach(), start)
    assert torch.equal(opt.ema.view(torch.int32), start.view(torch.int32))


def test_validation_and_switching_off():
    from ddp_amd.optim import FusedSGD
    model = _model()
    opt = FusedSGD(model.parameters(), lr=0.1)
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            opt.set_ema(bad)
    assert opt.ema_decay is None
    with pytest.raises(RuntimeError):
        opt.swap_ema()
    opt.set_ema(0.9)
    ptr = opt.ema.data_ptr()
    opt.set_ema(None)
    assert opt.ema_decay is None and "ema_decay" not in opt.param_groups[0]
    assert opt.updates_in_launch_only is False
    opt.set_ema(0.99)   # allocated once: the address survives
    assert opt.ema.data_ptr() == ptr and opt.param_groups[0]["ema_decay"] == 0.99


# -------------------------------------------------------------------------------- semantics
def test_skipped_step_leaves_the_ema_and_advances_the_schedule():
    from ddp_amd.optim import FusedSGD, LRSchedule
    model = _model()
    opt = FusedSGD(model.parameters(), lr=0.1, momentum=MOM, skip_nonfinite=True)
    opt.set_schedule(LRSchedule(base_lr=0.1, total_steps=6, warmup_steps=3, decay="cosine"))
    opt.set_ema(0.9)
    for s in range(2):   # (the warm-up's first rate is 0: the second step moves the weights)
        opt.zero_grad()
        _backward(model, s)
        opt.step()
    before, w = opt.ema.clone(), _weights(model)
    assert not torch.equal(before, torch.cat([p.reshape(-1) for p in w]))
    opt.zero_grad()
    _backward(model, 2)
    next(model.parameters()).grad.view(-1)[0] = float("inf")
    assert opt.lr_step == 2
    opt.step()
    assert int(opt.skipped_steps()) == 1 and opt.lr_step == 3
    assert torch.equal(opt.ema, before)
    assert all(torch.equal(a, b) for a, b in zip(_weights(model), w))


def test_accumulated_step_advances_the_ema_once():
    """train_model with accum_steps = 2 over 4 batches: two optimizer steps, two EMA steps."""
    from ddp_amd.engine import CrossEntropyLoss
    from ddp_amd.engine.trainer import train_model
    from ddp_amd.optim import FusedSGD
    model = _model()
    opt = FusedSGD(model.parameters(), lr=0.05, momentum=MOM)
    opt.set_ema(0.9)
    snaps = [_weights(model)]
    real = opt.step

    def step(*a, **k):
        out = real(*a, **k)
        snaps.append(_weights(model))
        return out
    opt.step = step
    train_model(model, [_batch(i) for i in range(4)], opt, CrossEntropyLoss(), 0, accum_steps=2,
                log=lambda *a: None)
    assert len(snaps) == 3
    for g, w in zip(opt.ema_state().values(), _recurrence(snaps, 0.9)):
        assert torch.equal(g, w)


# --------------------------------------------------------------------------------- plumbing
def test_plain_state_dict_is_unchanged():
    from ddp_amd.optim import FusedSGD, LARS
    model = _model()
    sd = FusedSGD(model.parameters(), lr=0.1, momentum=MOM, weight_decay=WD).state_dict()
    ref = torch.optim.SGD(model.parameters(), lr=0.1, momentum=MOM, weight_decay=WD).state_dict()
    assert set(sd) == {"state", "param_groups"}
    assert sd["param_groups"][0].keys() == ref["param_groups"][0].keys()
    assert "ema_decay" not in sd["param_groups"][0]
    on = LARS(model.parameters(), lr=0.1)
    on.set_ema(0.75)
    sd = on.state_dict()
    assert sd["param_groups"][0]["ema_decay"] == 0.75 and set(sd) == {"state", "param_groups"}
    other = LARS(_model(1).parameters(), lr=0.1)
    other.load_state_dict(sd)
    assert other.ema_decay == 0.75 and other.updates_in_launch_only


def _trained(decay=0.9, steps=2):
    from ddp_amd.optim import FusedSGD
    model = _model()
    opt = FusedSGD(model.parameters(), lr=0.05, momentum=MOM)
    if decay is not None:
        opt.set_ema(decay)
    for s in range(steps):
        opt.zero_grad()
        _backward(model, s)
        opt.step()
    return model, opt


def test_checkpoint_round_trip(tmp_path):
    from ddp_amd.optim import FusedSGD
    from ddp_amd.utils import load_checkpoint, save_checkpoint
    model, opt = _trained()
    path = str(tmp_path / "ck.pt")
    save_checkpoint(path, model, opt)
    obj = torch.load(path, weights_only=True)
    names = [k for k, _ in model.named_parameters()]
    assert list(obj["ema_state_dict"]) == names          # the reference keys, no BN buffers
    assert set(names) <= set(obj["model"])
    for k, p in model.named_parameters():
        assert not torch.equal(obj["ema_state_dict"][k], p.detach())
    # the flag given again on resume
    m2 = _model(1)
    o2 = FusedSGD(m2.parameters(), lr=0.05, momentum=MOM)
    load_checkpoint(path, m2, o2, ema_decay=0.9)
    assert torch.equal(o2.ema, opt.ema)
    # no flag: the saved optimizer state switches it on
    m3 = _model(2)
    o3 = FusedSGD(m3.parameters(), lr=0.05, momentum=MOM)
    load_checkpoint(path, m3, o3)
    assert o3.ema_decay == 0.9 and torch.equal(o3.ema, opt.ema)
    # a checkpoint written under DDP names: the module. prefix is stripped, as for the weights
    obj["model"] = {"module." + k: v for k, v in obj["model"].items()}
    obj["ema_state_dict"] = {"module." + k: v for k, v in obj["ema_state_dict"].items()}
    torch.save(obj, path)
    m4 = _model(3)
    o4 = FusedSGD(m4.parameters(), lr=0.05, momentum=MOM)
    load_checkpoint(path, m4, o4, ema_decay=0.9)
    assert torch.equal(o4.ema, opt.ema)
    assert all(torch.equal(a, b) for a, b in zip(_weights(m4), _weights(model)))


def test_ddp_wrapped_model_saves_the_reference_keys(tmp_path):
    """A wrapper with a ``module`` attribute: the EMA goes under the inner model's keys."""
    from ddp_amd.utils import save_checkpoint
    model, opt = _trained()
    wrapped = torch.nn.Module()
    wrapped.module = model
    path = str(tmp_path / "ck.pt")
    save_checkpoint(path, wrapped, opt)
    obj = torch.load(path, weights_only=True)
    assert list(obj["ema_state_dict"]) == [k for k, _ in model.named_parameters()]


def test_resume_without_an_ema_seeds_it_from_the_weights(tmp_path):
    from ddp_amd.optim import FusedSGD
    from ddp_amd.utils import load_checkpoint, save_checkpoint
    model, opt = _trained(decay=None)
    path = str(tmp_path / "ck.pt")
    save_checkpoint(path, model, opt)
    assert "ema_state_dict" not in torch.load(path, weights_only=True)
    m2 = _model(1)
    o2 = FusedSGD(m2.parameters(), lr=0.05, momentum=MOM)
    o2.set_ema(0.9)   # (seeded from the wrong weights first: the load must seed it again)
    load_checkpoint(path, m2, o2, ema_decay=0.9)
    for e, p in zip(o2.ema_state().values(), model.parameters()):
        assert torch.equal(e, p.detach())


def test_swap_and_context_manager():
    model, opt = _trained()
    w, e = _weights(model), [v.clone() for v in opt.ema_state().values()]
    with opt.ema_weights():
        assert all(torch.equal(a, b) for a, b in zip(_weights(model), e))
        assert all(torch.equal(a, b) for a, b in zip(opt.ema_state().values(), w))
    assert all(torch.equal(a, b) for a, b in zip(_weights(model), w))
    assert all(torch.equal(a, b) for a, b in zip(opt.ema_state().values(), e))
    state = opt.ema_state(model)
    assert list(state) == [k for k, _ in model.named_parameters()]
    opt.load_ema_state({k: v + 1 for k, v in state.items()}, model)
    assert all(torch.equal(a, b + 1) for a, b in zip(opt.ema_state().values(), e))


@pytest.mark.parametrize("bad", ["1.0", "-0.1", "1.5"])
def test_cli_refuses_a_bad_decay(bad):
    from ddp_amd.utils.cli import build_parser
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--ema-decay", bad])


def test_cli_default_is_off():
    from ddp_amd.utils.cli import build_parser
    assert build_parser().parse_args([]).ema_decay == 0.0
    assert build_parser().parse_args(["--ema-decay", "0.999"]).ema_decay == 0.999


def test_part1_prints_the_second_evaluation_line(tmp_path):
    metrics = str(tmp_path / "m.jsonl")
    r = subprocess.run([sys.executable, os.path.join(REPO, "part1", "main.py"), "--device", "cpu",
                        "--train-size", "64", "--test-size", "32", "--max-batches", "3",
                        "--global-batch", "8", "--threads", "2", "--ema-decay", "0.9",
                        "--metrics", metrics], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Test set")]
    assert len(lines) == 2, r.stdout
    assert lines[0].startswith("Test set: Average loss: ")
    assert lines[1].startswith("Test set (EMA): Average loss: ") and "Accuracy: " in lines[1]
    assert lines[0].split(":", 1)[1].split(",")[1].split("/")[1] == \
        lines[1].split(":", 1)[1].split(",")[1].split("/")[1]
    import json
    recs = [json.loads(ln) for ln in open(metrics)]
    assert recs and all(rec["ema_decay"] == 0.9 for rec in recs if rec.get("event") == "iter")


# --------------------------------------------------------------------------------- refusals
def test_sharded_and_element_updates_refuse_the_ema():
    from ddp_amd.optim import FusedSGD
    from ddp_amd.optim.arena import ParamArena
    from ddp_amd.parallel.zero import ShardedBf16Update, ShardedUpdate, arena_buckets

    class Comm:
        world, rank = 2, 0

    model = _model()
    arena = ParamArena(list(model.parameters()))
    opt = FusedSGD(model.parameters(), lr=0.1)
    opt.set_ema(0.9)
    buckets = arena_buckets(arena, [2])
    for cls in (ShardedUpdate, ShardedBf16Update):
        with pytest.raises(ValueError, match='update="allreduce"'):
            cls(arena, opt, Comm(), buckets)
    with pytest.raises(ValueError, match='update="allreduce"'):
        opt.step_elements(0, 64)
    with pytest.raises(RuntimeError, match="EMA"):
        opt.register_in_backward()
    opt.set_ema(None)
    opt.arena.grad.zero_()
    opt.step_elements(0, 64)   # off again: accepted


def test_train_step_keeps_the_update_out_of_the_backward(monkeypatch):
    """TrainStep.opt_in_bwd with a stand-in fused optimizer and device loader: True for the
    plain optimizer where SGD in the backward is allowed, False with the EMA on."""
    from ddp_amd.engine import step as st

    class Loader:
        device = "cpu"

        def cursor_advance(self, m):
            return (0, m)

    class Opt:
        _fused = True
        updates_in_launch_only = False

        def zero_grad(self):
            pass

        def register_in_backward(self):
            pass

    monkeypatch.delenv("DDP_AMD_SGD_IN_BWD", raising=False)
    monkeypatch.delenv("DDP_AMD_EMULATE_COMM", raising=False)
    monkeypatch.delenv("DDP_AMD_EMULATE_COMM_GBPS", raising=False)
    model, crit = torch.nn.Linear(2, 2), torch.nn.CrossEntropyLoss()
    assert st.TrainStep(model, Opt(), crit, Loader()).opt_in_bwd is True
    on = Opt()
    on.updates_in_launch_only = True
    assert st.TrainStep(model, on, crit, Loader()).opt_in_bwd is False


# ------------------------------------------------------------------------------------- Gloo
def test_gloo_ddp_ema_is_identical_on_both_ranks():
    from dist_helpers import run_workers
    from ema_dist_worker import ddp_ema_worker
    decay = 0.9
    out = run_workers(ddp_ema_worker, 2, 3, 4, decay)
    for r, v in out.items():
        assert "error" not in v, v.get("error")
        assert v["consistent"]
    assert torch.equal(out[0]["ema"].view(torch.int32), out[1]["ema"].view(torch.int32))
    assert torch.equal(out[0]["snaps"], out[1]["snaps"])
    snaps = [[s] for s in out[0]["snaps"]]
    assert len(snaps) == 4
    want = _recurrence(snaps, decay)[0]
    assert torch.equal(out[0]["ema"], want)
    assert not torch.equal(want, snaps[0][0]) and not torch.equal(want, snaps[-1][0])
