"""Muon on the CPU (optim/muon.py, utils/cli.py): the CPU class is the oracle of the Muon kernels
and the optimizer of the Gloo paths."""
import copy

import pytest
import torch

from ddp_amd.optim import FusedSGD, Muon
from ddp_amd.optim.muon import newton_schulz

SHAPES = [(32, 96), (96, 32)]
# Extreme singular values of O for the randn input _d(shape), measured. The Newton-Schulz iteration in
# fp64 with no bf16 rounding gives 0.681846 .. 1.036084 (32 x 96) and 0.681916 .. 1.062344 (96 x 32):
# the band, rounded outwards in the fifth digit. The bf16 chain of the CPU rule gives 0.679502 ..
# 1.043171 and 0.678985 .. 1.061484, at most 0.007087 outside the fp64 band: the deviation, rounded
# up to 0.008.
FP64_BAND = {(32, 96): (0.68184, 1.03609), (96, 32): (0.68191, 1.06235)}
BF16_DEVIATION = 0.008


def _d(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(0))


def _mm64(a, b):
    return a.double() @ b.double()


@pytest.mark.parametrize("shape", SHAPES)
def test_orthogonalisation(shape):
    d = _d(shape)
    ideal = torch.linalg.svdvals(newton_schulz(d, matmul=_mm64, keep=lambda x: x.double()))
    sv = torch.linalg.svdvals(newton_schulz(d).double())
    print(f"fp64 iteration {float(ideal.min()):.4f} .. {float(ideal.max()):.4f}; bf16 chain "
          f"{float(sv.min()):.4f} .. {float(sv.max()):.4f}")
    lo, hi = FP64_BAND[shape]
    assert lo <= float(ideal.min()) <= lo + 2e-5 and hi - 2e-5 <= float(ideal.max()) <= hi
    assert lo - BF16_DEVIATION <= float(sv.min()) and float(sv.max()) <= hi + BF16_DEVIATION


def _mm_exact(a, b):
    """The fp32 matmul rounded once: bf16 x bf16 products are exact in fp64 and a sum of a few
    hundred of them keeps 29 spare bits, so the result does not depend on the order of the sum."""
    return (a.double() @ b.double()).float()


@pytest.mark.parametrize("shape", SHAPES)
def test_invariances(shape):
    """Columns of the matrix [K][rest] permuted (the arena's [K][R][S][C] against [K][C][R][S])
    permute O's columns bit for bit, and zero padding changes no bit of the unpadded block. The
    permutation reorders the sums of X X^T (wide) or of A A and B X (tall), and an fp32 sum
    depends on its order: with torch.matmul 3 of 16 randn inputs gave an O that differed in
    6 .. 1251 elements. What the rule itself owes is checked with a matmul whose sums do not
    depend on the order (_mm_exact): orientation, normalisation and every store point commute
    with the permutation."""
    d = _d(shape)
    perm = torch.randperm(shape[1], generator=torch.Generator().manual_seed(1))
    O = newton_schulz(d, matmul=_mm_exact)
    assert torch.equal(newton_schulz(d[:, perm].contiguous(), matmul=_mm_exact), O[:, perm])
    padded = torch.zeros(shape[0] + 5, shape[1] + 9)
    padded[:shape[0], :shape[1]] = d
    assert torch.equal(newton_schulz(padded)[:shape[0], :shape[1]], newton_schulz(d))


def _params(seed=2):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in [(8, 3, 3, 3), (8,), (10, 8)]]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g)
    return ps


def test_pass_through():
    """Two steps: the 1-D and 2-D tensors and their momentum are FusedSGD's bit for bit."""
    kw = dict(lr=0.02, momentum=0.95, nesterov=True, weight_decay=1e-4)
    a, b = _params(), _params()
    mu, sgd = Muon(a, **kw), FusedSGD(b, **kw)
    assert mu.param_groups[0]["ortho"] == [0]
    for _ in range(2):
        mu.step()
        sgd.step()
    for i in (1, 2):
        assert torch.equal(a[i], b[i]) and torch.equal(mu.state[a[i]]["momentum_buffer"],
                                                       sgd.state[b[i]]["momentum_buffer"])


def test_state_dict_round_trip():
    a, b = _params(), _params()
    one, two = Muon(a, lr=0.02, ns_steps=4), Muon(b, lr=0.5, nesterov=False, ortho=[])
    one.step()
    sd = copy.deepcopy(one.state_dict())  # (a state dict shares the optimizer's tensors)
    assert {"ortho", "ns_steps", "nesterov", "momentum"} <= set(sd["param_groups"][0])
    assert set(sd["state"][0]) == {"momentum_buffer"}
    two.load_state_dict(sd)
    g = two.param_groups[0]
    assert (g["ortho"], g["ns_steps"], g["nesterov"], g["lr"]) == ([0], 4, True, 0.02)
    for p, q in zip(a, b):
        q.data.copy_(p.data)
    one.step()
    two.step()
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_cli_builds_muon():
    from ddp_amd.utils.cli import build_parser, optimizer_from_args
    args = build_parser().parse_args(["--optimizer", "muon", "--lr", "0.02", "--muon-ns-steps",
                                      "3", "--no-decay-1d"])
    opt = optimizer_from_args(args, _params(), args.lr)
    g = opt.param_groups[0]
    assert type(opt) is Muon and opt.metrics_name == "muon" and opt.updates_in_launch_only
    assert (g["momentum"], g["nesterov"], g["ns_steps"], g["weight_decay"]) == (0.95, True, 3, 1e-4)
    assert g["ortho"] == [0] and g["no_decay"] == [1]
    with pytest.raises(ValueError, match='Muon.*update="allreduce"'):
        opt.step_elements(0, 8)
    with pytest.raises(RuntimeError, match="Muon"):
        opt.register_in_backward()
