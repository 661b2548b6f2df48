"""Gradient accumulation (--accum-steps K), the parts that need no GPU: the flag, the schedule
length and the linear scaling rule over the effective batch, the epoch plan of the captured
loop, and the eager loop against a hand-written torch loop."""
import copy
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(*argv):
    from ddp_amd.utils.cli import parse_all
    return parse_all(list(argv), distributed=False)


# ---------------------------------------------------------------------------------------- CLI
def test_cli_default_is_one():
    assert _args().accum_steps == 1
    assert _args("--accum-steps", "4").accum_steps == 4


@pytest.mark.parametrize("bad", ["0", "-2", "x"])
def test_cli_rejects_non_positive(bad, capsys):
    with pytest.raises(SystemExit) as e:
        _args("--accum-steps", bad)
    assert e.value.code == 2
    assert "--accum-steps" in capsys.readouterr().err


def test_schedule_counts_optimizer_steps_and_lr_scales_by_effective_batch():
    from ddp_amd.utils.cli import lr_schedule_from_args
    a = _args("--accum-steps", "4", "--global-batch", "256", "--lr-ref-batch", "256",
              "--lr-schedule", "cosine", "--warmup-steps", "2", "--epochs", "3")
    # 10 loader batches per epoch -> 2 groups of 4 + one of 2 = 3 optimizer steps per epoch
    lr, sched = lr_schedule_from_args(a, 10)
    assert lr == pytest.approx(0.1 * 4)
    assert sched.table().numel() == 9
    # the same run without accumulation: 30 steps, lr not scaled
    b = _args("--global-batch", "256", "--lr-ref-batch", "256", "--lr-schedule", "cosine",
              "--warmup-steps", "2", "--epochs", "3")
    lr1, sched1 = lr_schedule_from_args(b, 10)
    assert lr1 == pytest.approx(0.1) and sched1.table().numel() == 30
    # no schedule asked for: only the scaled rate
    c = _args("--accum-steps", "2", "--lr-ref-batch", "128", "--global-batch", "64")
    assert lr_schedule_from_args(c, 10) == (pytest.approx(0.1), None)


# ----------------------------------------------------------------------------------- epoch plan
@pytest.mark.parametrize("n,batch,K,max_batches,want", [
    (1000, 64, 4, None, (3, 3, 40)),    # 15 full batches: 3 replays, 3 left over, tail 40
    (1024, 64, 4, None, (4, 0, 0)),     # divides evenly: replays only
    (1000, 64, 1, None, (15, 0, 40)),   # K = 1: graph_epoch_plan
    (1000, 64, 16, None, (0, 15, 40)),  # fewer full batches than K: one eager step of 16
    (1000, 64, 4, 6, (1, 2, 0)),        # max_batches cuts inside the second group
    (1000, 64, 4, 16, (3, 3, 40)),      # max_batches reaches the partial batch
    (1000, 64, 4, 15, (3, 3, 0)),       # ... stops just before it
    (40, 64, 4, None, (0, 0, 40)),      # only a partial batch
])
def test_accum_epoch_plan(n, batch, K, max_batches, want):
    from ddp_amd.engine.trainer import accum_epoch_plan, graph_epoch_plan
    got = accum_epoch_plan(n, batch, K, max_batches)
    assert got == want
    # every loader batch of the epoch is consumed exactly once
    nfull, tail = graph_epoch_plan(n, batch, max_batches)
    assert got[0] * K + got[1] == nfull and got[2] == tail


# ----------------------------------------------------------------------------------- eager loop
def test_train_model_matches_hand_written_loop():
    """train_model(accum_steps=3) over 7 batches of 8 (two groups of 3 and a leftover of 1)
    against the usual PyTorch idiom, (loss / m).backward() per micro-batch and one step per
    group: parameters, BatchNorm buffers and momentum buffers bit for bit."""
    from ddp_amd import SEED
    from ddp_amd.data import SyntheticCIFAR10
    from ddp_amd.data.loader import CPULoader
    from ddp_amd.engine import CrossEntropyLoss
    from ddp_amd.engine.trainer import train_model
    from ddp_amd.models import VGG11
    from ddp_amd.optim import FusedSGD
    torch.manual_seed(SEED)
    model = VGG11()
    ref = copy.deepcopy(model)
    ds = SyntheticCIFAR10(train=True, seed=SEED, n=56)
    hp = dict(lr=0.1, momentum=0.9, weight_decay=1e-4)

    opt = FusedSGD(model.parameters(), **hp)
    lines, records = [], []

    class Sink:
        def log(self, **kw):
            records.append(kw)
    stats = train_model(model, CPULoader(ds, 8, train=True, shard=False), opt, CrossEntropyLoss(),
                        0, "cpu", log=lines.append, metrics=Sink(), accum_steps=3)
    assert len(stats["iter_ns"]) == 3
    assert [r["accum"] for r in records] == [3, 3, 1]
    assert [r["batch"] for r in records] == [0, 1, 2]

    ropt = torch.optim.SGD(ref.parameters(), **hp)
    batches = list(CPULoader(ds, 8, train=True, shard=False))
    assert len(batches) == 7
    for group in (batches[0:3], batches[3:6], batches[6:7]):
        ropt.zero_grad()
        for x, y in group:
            loss = torch.nn.functional.cross_entropy(ref(x), y)
            (loss / len(group)).backward()
        ropt.step()

    sd, rsd = model.state_dict(), ref.state_dict()
    assert list(sd) == list(rsd)
    for k in sd:
        assert torch.equal(sd[k], rsd[k]), k
    for p, rp in zip(model.parameters(), ref.parameters()):
        assert torch.equal(opt.state[p]["momentum_buffer"], ropt.state[rp]["momentum_buffer"])


def test_train_model_default_is_the_plain_loop():
    """accum_steps=1 takes the loop that was there before: no ``accum`` field in the metrics."""
    from ddp_amd import SEED
    from ddp_amd.data import SyntheticCIFAR10
    from ddp_amd.data.loader import CPULoader
    from ddp_amd.engine import CrossEntropyLoss
    from ddp_amd.engine.trainer import train_model
    from ddp_amd.models import VGG11
    from ddp_amd.optim import FusedSGD
    torch.manual_seed(SEED)
    model = VGG11()
    records = []

    class Sink:
        def log(self, **kw):
            records.append(kw)
    train_model(model, CPULoader(SyntheticCIFAR10(True, seed=SEED, n=16), 8, shard=False),
                FusedSGD(model.parameters(), lr=0.1), CrossEntropyLoss(), 0, "cpu",
                log=lambda s: None, metrics=Sink(), accum_steps=1)
    assert len(records) == 2 and all("accum" not in r for r in records)


# ------------------------------------------------------------------------------------ the main
def _part1(*extra):
    r = subprocess.run([sys.executable, os.path.join(REPO, "part1", "main.py"), "--device", "cpu",
                        "--train-size", "640", "--test-size", "64", "--global-batch", "8",
                        "--threads", "2", *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_part1_counts_optimizer_steps(tmp_path):
    """--accum-steps 2 --max-batches 8: --max-batches counts loader batches, so the epoch has 4
    iterations (the metrics sink has one record each, ``accum`` 2); with 80 batches the 40
    iterations print the reference's lines at iteration 20 and 40."""
    import json
    path = str(tmp_path / "m.jsonl")
    _part1("--accum-steps", "2", "--max-batches", "8", "--metrics", path)
    recs = [json.loads(l) for l in open(path) if l.strip()]
    iters = [r for r in recs if r.get("event") == "iter"]
    assert [r["batch"] for r in iters] == [0, 1, 2, 3]
    assert all(r["accum"] == 2 for r in iters)
    out = _part1("--accum-steps", "2", "--max-batches", "80", "--no-test")
    assert sum(l.startswith("[1,    20] loss: ") for l in out) == 1
    assert sum(l.startswith("[1,    40] loss: ") for l in out) == 1
    assert not any(l.startswith("[1,    60] loss: ") for l in out)
    assert any(l.startswith("Total time for 1-39 iteration in ns: ") for l in out)


def test_part1_without_the_flag_keeps_its_format():
    out = _part1("--max-batches", "41")
    assert any(l.startswith("[1,    20] loss: ") for l in out)
    assert any(l.startswith("[1,    40] loss: ") for l in out)
    assert any(l.startswith("Total time for 1-39 iteration in ns: ") for l in out)
    assert any(l.startswith("Average time for 1-39 iteration in ns: ") for l in out)
    assert any(l.startswith("Test set: Average loss: ") and "Accuracy: " in l and "/64 (" in l
               for l in out)
