"""Learning-rate schedules (optim/schedule.py, FusedSGD.set_schedule) on the CPU: the table is
torch.optim.lr_scheduler's values, the CPU optimizer applies exactly table[k] at step k, the
schedule survives a checkpoint, DDP replicas stay identical, and the mains' default output is
what it was before the schedule flags existed."""
import json
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "part1_cpu_default_stdout.txt")

# one fp32 rounding of a float64 closed form vs torch's float64 chained form: ~8 fp32 ulps
RTOL = 1e-6


def _torch_lrs(make_sched, base_lr, n):
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=base_lr)
    sched = make_sched(opt)
    out = []
    for _ in range(n):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return torch.tensor(out, dtype=torch.float64)


def _check(schedule, ref):
    t = schedule.table()
    assert t.dtype == torch.float32 and t.numel() == schedule.total_steps
    assert torch.allclose(t.double(), ref, rtol=RTOL, atol=0.0), (t, ref)
    for k in (0, 1, schedule.total_steps - 1):
        assert schedule.lr_at(k) == float(t[k])


def test_warmup_cosine_matches_torch():
    from ddp_amd.optim import LRSchedule
    from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR, SequentialLR
    base, n, w = 0.4, 50, 7
    s = LRSchedule(base, n, warmup_steps=w, warmup_start_factor=0.1, decay="cosine", min_lr=0.01)
    ref = _torch_lrs(lambda o: SequentialLR(o, [
        LinearLR(o, start_factor=0.1, end_factor=1.0, total_iters=w),
        CosineAnnealingLR(o, T_max=n - w, eta_min=0.01)], milestones=[w]), base, n)
    _check(s, ref)
    # the default warm-up starts at 0 (torch's LinearLR cannot): exact end points
    z = LRSchedule(base, n, warmup_steps=w, decay="cosine")
    assert z.lr_at(0) == 0.0 and z.lr_at(w) == float(torch.tensor(base, dtype=torch.float32))


def test_step_linear_constant_match_torch():
    from ddp_amd.optim import LRSchedule
    from torch.optim.lr_scheduler import LinearLR, MultiStepLR
    base, n = 0.1, 30
    s = LRSchedule(base, n, decay="step", milestones=(20, 10), gamma=0.5)
    _check(s, _torch_lrs(lambda o: MultiStepLR(o, milestones=[10, 20], gamma=0.5), base, n))
    lin = LRSchedule(base, n, decay="linear", min_lr=0.02)
    _check(lin, _torch_lrs(lambda o: LinearLR(o, start_factor=1.0, end_factor=0.2,
                                              total_iters=n), base, n))
    c = LRSchedule(base, n)  # warmup_steps=0, constant: exact
    assert torch.equal(c.table(), torch.full((n,), base, dtype=torch.float32))


def test_clamp_and_no_warmup():
    from ddp_amd.optim import LRSchedule
    s = LRSchedule(0.2, 10, warmup_steps=0, decay="cosine")
    assert s.lr_at(0) == float(torch.tensor(0.2, dtype=torch.float32))
    assert s.lr_at(10) == s.lr_at(9) == s.lr_at(10 ** 6) == float(s.table()[-1])
    assert s.lr_at(9) > 0.0
    with pytest.raises(ValueError):
        LRSchedule(0.1, 10, decay="exponential")
    with pytest.raises(ValueError):
        LRSchedule(0.1, 4, warmup_steps=5)


def test_schedule_state_dict_is_plain():
    from ddp_amd.optim import LRSchedule
    s = LRSchedule(0.3, 12, warmup_steps=3, decay="step", milestones=(6, 9), gamma=0.2)
    sd = s.state_dict()

    def plain(v):
        return isinstance(v, (int, float, str)) or (isinstance(v, list) and all(map(plain, v)))
    assert all(plain(v) for v in sd.values())
    t = LRSchedule(1.0, 1).load_state_dict(json.loads(json.dumps(sd)))
    assert torch.equal(t.table(), s.table())


def _mlp(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(12, 33), torch.nn.ReLU(), torch.nn.Linear(33, 5))


def _batches(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(6, 12, generator=g), torch.randint(0, 5, (6,), generator=g))
            for _ in range(n)]


def _sched():
    from ddp_amd.optim import LRSchedule
    return LRSchedule(0.2, 6, warmup_steps=2, warmup_start_factor=0.25, decay="cosine")


def _flat(model):
    return torch.cat([p.detach().reshape(-1).clone() for p in model.parameters()])


def test_cpu_fused_sgd_matches_hand_set_lr():
    """8 steps of a 6-entry table: the last two steps use the clamped last entry."""
    from ddp_amd.optim import FusedSGD
    table = _sched().table()
    a, b = _mlp(), _mlp()
    oa = FusedSGD(a.parameters(), lr=0.2, momentum=0.9, weight_decay=1e-4)
    oa.set_schedule(_sched())
    ob = torch.optim.SGD(b.parameters(), lr=0.2, momentum=0.9, weight_decay=1e-4)
    for k, (x, y) in enumerate(_batches(8)):
        lr = float(table[min(k, 5)])
        assert oa.lr_step == k and oa.current_lr() == lr
        ob.param_groups[0]["lr"] = lr
        for m, o in ((a, oa), (b, ob)):
            o.zero_grad()
            torch.nn.functional.cross_entropy(m(x), y).backward()
            o.step()
        assert oa.param_groups[0]["lr"] == lr
    assert torch.equal(_flat(a), _flat(b))
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(oa.state[p]["momentum_buffer"], ob.state[q]["momentum_buffer"])
    # detached: the param group's learning rate is the host's again
    oa.set_schedule(None)
    oa.param_groups[0]["lr"] = 0.5
    assert oa.current_lr() == 0.5


def test_cpu_step_elements_matches_hand_set_lr():
    """The ZeRO-1 CPU path (element ranges of the flat arena; two ranges per step, the second
    one ends the step)."""
    from ddp_amd.optim import FusedSGD, ParamArena
    table = _sched().table()
    a, b = _mlp(), _mlp()
    arena = ParamArena(a.parameters())
    oa = FusedSGD(a.parameters(), lr=0.2, momentum=0.9, weight_decay=1e-4)
    assert oa.arena is arena
    oa.set_schedule(_sched())
    ob = torch.optim.SGD(b.parameters(), lr=0.2, momentum=0.9, weight_decay=1e-4)
    cut = arena.offsets[2]
    for k, (x, y) in enumerate(_batches(8)):
        ob.param_groups[0]["lr"] = float(table[min(k, 5)])
        arena.zero_grad()
        ob.zero_grad()
        torch.nn.functional.cross_entropy(a(x), y).backward()
        torch.nn.functional.cross_entropy(b(x), y).backward()
        oa.step_elements(cut, arena.total, lr_advance=False)
        assert oa.lr_step == k
        oa.step_elements(0, cut)
        assert oa.lr_step == k + 1
        ob.step()
    assert torch.equal(_flat(a), _flat(b))


def test_checkpoint_round_trip(tmp_path):
    from ddp_amd.optim import FusedSGD
    from ddp_amd.utils import load_checkpoint, save_checkpoint
    batches = _batches(6)

    def run(model, opt, bs):
        for x, y in bs:
            opt.zero_grad()
            torch.nn.functional.cross_entropy(model(x), y).backward()
            opt.step()

    a = _mlp()
    oa = FusedSGD(a.parameters(), lr=0.2, momentum=0.9, weight_decay=1e-4)
    oa.set_schedule(_sched())
    run(a, oa, batches)

    b = _mlp()
    ob = FusedSGD(b.parameters(), lr=0.2, momentum=0.9, weight_decay=1e-4)
    ob.set_schedule(_sched())
    run(b, ob, batches[:3])
    path = str(tmp_path / "ck.pt")
    save_checkpoint(path, b, ob)

    c = _mlp(seed=7)  # fresh model and optimizer, no schedule attached by hand
    oc = FusedSGD(c.parameters(), lr=0.9, momentum=0.9, weight_decay=1e-4)
    load_checkpoint(path, c, oc)
    assert oc.lr_step == 3 and oc.schedule is not None
    assert torch.equal(oc.schedule.table(), _sched().table())
    run(c, oc, batches[3:])
    assert oc.lr_step == 6
    assert torch.equal(_flat(a), _flat(c))
    for p, q in zip(a.parameters(), c.parameters()):
        assert torch.equal(oa.state[p]["momentum_buffer"], oc.state[q]["momentum_buffer"])


def test_gloo_ddp_with_warmup_schedule():
    from dist_helpers import run_workers
    from lr_dist_worker import ddp_schedule_worker, schedule_kwargs
    from ddp_amd.optim import LRSchedule
    steps = 5  # one more than the table: the last step runs on the clamped entry
    out = run_workers(ddp_schedule_worker, 2, steps, 4)
    for r, v in out.items():
        assert "error" not in v, v.get("error")
        assert v["schedule_consistent"] and v["by_hand_consistent"]
        assert v["schedule_lr_step"] == steps
    table = LRSchedule(**schedule_kwargs()).table()
    assert out[0]["schedule_lrs"] == [float(table[min(k, 3)]) for k in range(steps)]
    assert out[0]["schedule_lrs"] == out[0]["by_hand_lrs"]
    assert torch.equal(out[0]["schedule"], out[1]["schedule"])
    assert torch.equal(out[0]["schedule"], out[0]["by_hand"])


def test_cli_flags_parse():
    from ddp_amd.utils.cli import lr_schedule_from_args, parse_all
    a = parse_all([], distributed=False)
    assert a.lr == 0.1 and a.lr_schedule is None and a.warmup_steps == 0
    assert a.lr_milestones == [] and a.lr_gamma == 0.1 and a.min_lr == 0.0
    assert a.lr_ref_batch is None
    assert lr_schedule_from_args(a, 10) == (0.1, None)
    a = parse_all(["--lr", "0.2", "--lr-schedule", "step", "--warmup-steps", "5",
                   "--lr-milestones", "30,60", "--lr-gamma", "0.5", "--min-lr", "0.001",
                   "--lr-ref-batch", "256", "--global-batch", "1024", "--epochs", "3"],
                  distributed=False)
    lr, s = lr_schedule_from_args(a, 40)
    assert lr == pytest.approx(0.8)
    assert s.total_steps == 120 and s.warmup_steps == 5 and s.decay == "step"
    assert s.milestones == [30, 60] and s.gamma == 0.5 and s.base_lr == pytest.approx(0.8)
    # a warm-up alone attaches a (constant-after-warm-up) schedule
    a = parse_all(["--warmup-steps", "4"], distributed=False)
    lr, s = lr_schedule_from_args(a, 10)
    assert s is not None and s.decay == "constant" and s.lr_at(0) == 0.0


MAIN_ARGS = ["--device", "cpu", "--max-batches", "3", "--train-size", "64", "--test-size", "16",
             "--global-batch", "8", "--threads", "1"]


def _run_main(extra, tmp_path=None):
    r = subprocess.run([sys.executable, os.path.join(REPO, "part1", "main.py")] + MAIN_ARGS + extra,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_part1_default_output_unchanged(tmp_path):
    """Default flags: stdout is byte-identical to the recorded output of the same command
    before the schedule flags existed, and the metrics records carry no ``lr`` field; with a
    schedule the records log the table's values."""
    m0, m1 = str(tmp_path / "m0.jsonl"), str(tmp_path / "m1.jsonl")
    out = _run_main(["--metrics", m0])
    with open(GOLDEN) as f:
        assert out == f.read()
    recs = [json.loads(l) for l in open(m0)]
    assert len(recs) == 3 and all("lr" not in r for r in recs)
    _run_main(["--metrics", m1, "--lr-schedule", "cosine", "--warmup-steps", "1", "--no-test"])
    from ddp_amd.optim import LRSchedule
    s = LRSchedule(0.1, 3, warmup_steps=1, decay="cosine")
    assert [json.loads(l)["lr"] for l in open(m1)] == [s.lr_at(k) for k in range(3)]
