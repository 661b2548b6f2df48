"""Label smoothing and mixup on the CPU path: the loss class against torch's fp64 formulas, the
lam table, the CPU loader's blend, the mains' flags, accumulation and two Gloo ranks."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------ the loss
@pytest.mark.parametrize("E,lam", [(0.1, 1.0), (0.0, 0.3), (0.1, 0.3), (0.1, 0.0)])
def test_loss_class_equals_torch_fp64(E, lam):
    """CrossEntropyLoss(label_smoothing=E)(logits, y, (y2, lam)) on fp64 logits equals
    lam CE(y) + (1 - lam) CE(y2) with torch's label_smoothing, and the soft-target form
    mean_b (lse - sum_j t_j z_j) of the kernels."""
    from ddp_amd.engine import CrossEntropyLoss
    g = torch.Generator().manual_seed(3)
    B, J = 6, 10
    z = torch.randn(B, J, generator=g, dtype=torch.float64) * 3
    y = torch.randint(0, J, (B,), generator=g)
    y2 = y.flip(0)
    lam_t = torch.tensor([lam], dtype=torch.float32)
    lam32 = float(lam_t)
    crit = CrossEntropyLoss(label_smoothing=E)
    got = crit(z, y, (y2, lam_t))
    want = lam32 * F.cross_entropy(z, y, label_smoothing=E) \
        + (1 - lam32) * F.cross_entropy(z, y2, label_smoothing=E)
    assert torch.allclose(got, want, rtol=1e-13, atol=1e-13)
    t = (1 - E) * (lam32 * F.one_hot(y, J) + (1 - lam32) * F.one_hot(y2, J)).double() + E / J
    form = (torch.logsumexp(z, 1) - (t * z).sum(1)).mean()
    assert torch.allclose(got, form, rtol=1e-12, atol=1e-12)
    # smoothing alone, and the default: torch's own losses
    assert torch.equal(crit(z, y), F.cross_entropy(z, y, label_smoothing=E))
    assert torch.equal(CrossEntropyLoss()(z, y), F.cross_entropy(z, y))
    assert CrossEntropyLoss().soft() is None and CrossEntropyLoss().label_smoothing == 0.0


def test_loss_class_refuses_bad_smoothing():
    from ddp_amd.engine import CrossEntropyLoss
    for e in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="label_smoothing"):
            CrossEntropyLoss(label_smoothing=e)


# --------------------------------------------------------------------------------- the lam table
def test_lam_table():
    from ddp_amd.data import CPULoader, SyntheticCIFAR10, lam_table
    a = lam_table(7, 0, 0.2, 12)
    assert a.dtype == np.float32 and a.shape == (12,) and bool(((a >= 0) & (a <= 1)).all())
    assert np.array_equal(a, lam_table(7, 0, 0.2, 12))            # reproducible
    assert not np.array_equal(a, lam_table(7, 1, 0.2, 12))        # another epoch
    assert not np.array_equal(a, lam_table(8, 0, 0.2, 12))        # another dataset seed
    assert not np.array_equal(a, lam_table(7, 0, 0.4, 12))        # another alpha
    assert lam_table(7, 0, 0.0, 12) is None and lam_table(7, 0, 0, 12) is None
    ds = SyntheticCIFAR10(True, n=64)
    r0 = CPULoader(ds, 8, num_replicas=2, rank=0, mixup_alpha=0.2)
    r1 = CPULoader(ds, 8, num_replicas=2, rank=1, mixup_alpha=0.2)
    assert np.array_equal(r0.lam_table, r1.lam_table) and len(r0.lam_table) == 4  # no rank in it
    assert np.array_equal(r0.lam_table, lam_table(ds.seed, 0, 0.2, 4))
    first = r0.lam_table.copy()
    r0.set_epoch(1)
    assert not np.array_equal(first, r0.lam_table)
    off = CPULoader(ds, 8)
    assert off.lam_table is None and off.soft_targets() is None
    assert all(off.soft_targets() is None for _ in off)


def test_cpu_loader_mixes_with_the_reversed_batch():
    """x = bf16(lam a + (1 - lam) a reversed) in fp32 from the unmixed loader's batches, the
    labels untouched, the partners the labels reversed, lam the table's entry per batch."""
    from ddp_amd.data import CPULoader, SyntheticCIFAR10
    ds = SyntheticCIFAR10(True, n=20)  # batches of 8, 8 and a partial one of 4
    plain = list(CPULoader(ds, 8, shard=False))
    ld = CPULoader(ds, 8, shard=False, mixup_alpha=0.4)
    assert len(ld.lam_table) == 3
    for i, (x, y) in enumerate(ld):
        y2, lam = ld.soft_targets()
        a, ya = plain[i]
        assert torch.equal(y, ya) and torch.equal(y2, ya.flip(0))
        assert lam.dtype == torch.float32 and float(lam) == float(ld.lam_table[i])
        want = (lam * a + (1 - lam) * a.flip(0)).to(torch.bfloat16).float()
        assert torch.equal(x, want) and x.dtype == torch.float32
        assert not torch.equal(x, a)


# ------------------------------------------------------------------------------ the eager loop
def test_accumulated_cpu_step_equals_two_hand_run_micro_batches():
    """train_model(accum_steps=2) with both flags against two hand-run micro-batches mixed with
    table entries 0 and 1: parameters bit for bit; the metrics record lists both lam."""
    from ddp_amd import SEED
    from ddp_amd.data import CPULoader, SyntheticCIFAR10
    from ddp_amd.data.loader import augment_cpu
    from ddp_amd.engine import CrossEntropyLoss
    from ddp_amd.engine.trainer import train_model
    from ddp_amd.models import VGG11
    from ddp_amd.optim import FusedSGD
    torch.manual_seed(SEED)
    model = VGG11()
    ref = copy.deepcopy(model)
    E, A = 0.1, 0.2
    ds = SyntheticCIFAR10(True, seed=SEED, n=16)
    hp = dict(lr=0.1, momentum=0.9, weight_decay=1e-4)
    recs = []

    class Sink:
        def log(self, **kw):
            recs.append(kw)
    ld = CPULoader(ds, 8, shard=False, mixup_alpha=A)
    train_model(model, ld, FusedSGD(model.parameters(), **hp), CrossEntropyLoss(label_smoothing=E),
                0, "cpu", log=lambda s: None, metrics=Sink(), accum_steps=2)
    table = ld.lam_table
    assert len(recs) == 1 and recs[0]["accum"] == 2
    assert recs[0]["lam"] == [float(table[0]), float(table[1])]

    ropt = torch.optim.SGD(ref.parameters(), **hp)
    imgs, labels = ds.cpu_arrays()
    ropt.zero_grad()
    for j in range(2):
        idx = np.arange(8 * j, 8 * j + 8)
        lam = float(table[j])
        x = augment_cpu(imgs, idx, ds.seed, 0, True, lam=table[j])
        y = torch.from_numpy(labels[idx].astype(np.int64))
        out = ref(x)
        loss = lam * F.cross_entropy(out, y, label_smoothing=E) \
            + (1 - lam) * F.cross_entropy(out, y.flip(0), label_smoothing=E)
        (loss / 2).backward()
    ropt.step()
    for (n, p), rp in zip(model.named_parameters(), ref.parameters()):
        assert torch.equal(p, rp), n


def test_evaluation_stays_plain():
    """test_model with a smoothing criterion reports the plain mean CE."""
    from ddp_amd.data import CPULoader, SyntheticCIFAR10
    from ddp_amd.engine import CrossEntropyLoss
    from ddp_amd.engine.trainer import test_model as evaluate
    from ddp_amd.models import VGG11
    torch.manual_seed(5)
    model = VGG11()
    ld = CPULoader(SyntheticCIFAR10(False, n=16), 8, train=False, shard=False)
    a = evaluate(model, ld, CrossEntropyLoss(label_smoothing=0.3), log=lambda s: None)
    b = evaluate(model, ld, CrossEntropyLoss(), log=lambda s: None)
    assert a == b


# ------------------------------------------------------------------------------------ the main
def _part1(*extra, ok=True):
    r = subprocess.run([sys.executable, os.path.join(REPO, "part1", "main.py"), "--device", "cpu",
                        "--train-size", "640", "--test-size", "64", "--global-batch", "8",
                        "--threads", "2", *extra], capture_output=True, text=True, timeout=600)
    if ok:
        assert r.returncode == 0, r.stderr
    return r


def test_part1_runs_with_both_flags(tmp_path):
    path = str(tmp_path / "m.jsonl")
    out = _part1("--max-batches", "3", "--label-smoothing", "0.1", "--mixup-alpha", "0.2",
                 "--metrics", path).stdout.splitlines()
    assert any(l.startswith("Test set: Average loss: ") and "Accuracy: " in l and "/64 (" in l
               for l in out)
    from ddp_amd import SEED
    from ddp_amd.data import lam_table
    iters = [r for r in (json.loads(l) for l in open(path) if l.strip()) if r.get("event") == "iter"]
    table = lam_table(SEED, 0, 0.2, 80)
    assert [r["lam"] for r in iters] == [float(v) for v in table[:3]]
    # flags off: no lam in the records
    path2 = str(tmp_path / "n.jsonl")
    _part1("--max-batches", "2", "--no-test", "--metrics", path2)
    assert all("lam" not in json.loads(l) for l in open(path2) if l.strip())


@pytest.mark.parametrize("flags", [("--label-smoothing", "1.0"), ("--label-smoothing", "-0.1"),
                                   ("--mixup-alpha", "-1"), ("--mixup-alpha", "inf"),
                                   ("--mixup-alpha", "nan")])
def test_bad_flag_values_are_refused(flags):
    from ddp_amd.utils.cli import build_parser
    with pytest.raises(SystemExit):
        build_parser(distributed=False).parse_args(list(flags))


def test_bad_flag_value_message(capsys):
    from ddp_amd.utils.cli import build_parser
    with pytest.raises(SystemExit):
        build_parser(distributed=False).parse_args(["--label-smoothing", "1"])
    assert "--label-smoothing must be in [0, 1)" in capsys.readouterr().err
    args = build_parser(distributed=False).parse_args([])
    assert args.label_smoothing == 0.0 and args.mixup_alpha == 0.0


# --------------------------------------------------------------------------------- two ranks
def test_two_gloo_ranks_stay_identical_with_both_flags():
    from dist_helpers import run_workers
    from soft_targets_dist_worker import STEPS, soft_worker
    out = run_workers(soft_worker, 2, 8)
    for r in range(2):
        assert "error" not in out[r], out[r].get("error")
        assert out[r]["iters"] == STEPS and out[r]["consistent"] is True
    assert torch.equal(out[0]["params"], out[1]["params"])
    assert out[0]["lam"] == out[1]["lam"] == out[0]["table"][:STEPS] and len(out[0]["lam"]) == STEPS
