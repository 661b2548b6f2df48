"""Muon through optim.Muon on the GPU: stage, fifteen GEMM launches and the update chained, against
the CPU class (optim/muon.py newton_schulz, the oracle)."""
import json
import os
import subprocess
import sys

import pytest
import torch

import test_gpu_lars as gl
from ddp_amd.optim import Muon
from ddp_amd.optim.muon import newton_schulz
from exactness import FP32_EPS, assert_within

pytestmark = pytest.mark.gpu
DEV = "cuda"
# What reordering the accumulation can do to O on the inputs below: the largest per-element
# difference between the oracle with fp32 matmul and the same chain with fp64 matmul (identical
# bf16 store points), relative to the tensor's max |O|, over the three orthogonalised tensors and
# both steps, measured on the CPU (the test measures it again and prints it; profiles/muon.md):
# 1.786e-2, one bf16 ulp of an element of the 72 x 576 tensor. Four times it is allowed, tol =
# 7.14e-2 of max |O|: the GPU sums in yet another order, and a flipped bf16 rounding propagates
# through five iterations.
REORDER = 1.786e-2
MARGIN = 4.0
TOL = MARGIN * REORDER


def _rig(seed=3):
    """tests/test_gpu_lars.py _kernel_params plus one tall bare 4-D tensor (96 x 8 x 2 x 2)."""
    ps, specs = gl._kernel_params()
    ps.append(torch.nn.Parameter(torch.randn(96, 8, 2, 2, device=DEV)))
    opt = Muon(ps, lr=0.02, weight_decay=1e-2)
    for sp in specs:
        sp.maybe_pack()
    g = torch.Generator(device=DEV).manual_seed(seed)
    opt.momentum_buffer.copy_(0.1 * torch.randn(opt.arena.total, device=DEV, generator=g))
    return ps, specs, opt


def _mm64(a, b):
    return a.double() @ b.double()


def test_chained_bound(native_ext):
    ps, specs, opt = _rig()
    ortho = opt.param_groups[0]["ortho"]
    assert ortho == [0, 4, len(ps) - 1]
    a, measured = opt.arena, []
    view = lambda t, i: a.shaped(t, i).detach().cpu().float()  # noqa: E731
    for step in range(2):
        grads = [torch.randn(p.shape, device=DEV) for p in ps]
        gl._set_grads(ps, grads)
        p0 = [view(a.data, i) for i in range(len(ps))]
        m0 = [view(opt.momentum_buffer, i) for i in range(len(ps))]
        opt.step(zero_grad=True)
        torch.cuda.synchronize()
        assert not bool(a.grad.any())
        for i in ortho:
            g, K = grads[i].cpu().double(), ps[i].shape[0]
            m1 = 0.95 * m0[i].double() + g
            d = (0.95 * m1 + g).float().reshape(K, -1)
            O32, O64 = newton_schulz(d), newton_schulz(d, matmul=_mm64)
            got = opt.ortho_output(i).cpu().reshape(K, -1)
            scale = float(O32.abs().max())
            reorder = float((O32 - O64).abs().max()) / scale
            err = float((got - O32).abs().max()) / scale
            print(f"step {step} parameter {i}: reorder effect {reorder:.3e}, device against the "
                  f"oracle {err:.3e} of max |O| = {scale:.4f}")
            measured.append(reorder)
            assert err <= TOL, (step, i)
            # p and m against the rule run with the O the device stored
            s = opt._geometry(i)[5]
            want_p = p0[i].double() * (1 - 0.02 * 1e-2) - 0.02 * s * got.double().reshape(ps[i].shape)
            T = p0[i].abs().double() + 0.02 * s * got.abs().double().reshape(ps[i].shape)
            assert_within(view(a.data, i).reshape(-1), want_p.reshape(-1), (4 * FP32_EPS * T).reshape(-1),
                          what=f"parameter {i}: p")
            Tm = 0.95 * m0[i].abs().double() + g.abs()
            assert_within(view(opt.momentum_buffer, i).reshape(-1), m1.reshape(-1),
                          (2 * FP32_EPS * Tm).reshape(-1), what=f"parameter {i}: m")
    assert max(measured) == pytest.approx(REORDER, rel=1e-3), measured  # TOL is 4 x what was measured


def test_eager_equals_captured_deterministic(native_ext):
    """tests/muon_probe.py: 3 steps of VGG-11 at batch 32, the second one skipped by the guard
    inside the step; masters, momentum and the EMA are torch.equal between eager and replays."""
    env = dict(os.environ, DDP_AMD_DETERMINISTIC="1")
    env.pop("DDP_AMD_SGD_IN_BWD", None)
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "muon_probe.py")],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert len(res) == 12 and all(v is True for v in res.values()), res


def test_resnet50_step(native_ext):
    """One eager ResNet-50 step at 16 x 128 x 128 (tests/test_gpu_resnet.py): 1x1 expansion convs are
    tall (kind-2 items read through the transposed index), the 7x7 stem goes through tile items."""
    from ddp_amd.engine import CrossEntropyLoss
    from ddp_amd.models.resnet import resnet50
    torch.manual_seed(0)
    model = resnet50(num_classes=16).cuda()
    opt = Muon(model.parameters(), lr=0.02, weight_decay=1e-4)
    ortho = opt.param_groups[0]["ortho"]
    assert any(opt._geometry(i)[2] for i in ortho) and max(opt._geometry(i)[4] for i in ortho) == 4608
    p0 = opt.arena.data.clone()
    opt.zero_grad()
    loss = CrossEntropyLoss()(model(torch.randn(16, 3, 128, 128, device=DEV)), torch.randint(0, 16, (16,), device=DEV))
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert float(loss) == float(loss) and bool(torch.isfinite(opt.arena.data).all())
    for i in ortho:
        o, n = opt.arena.offsets[i], opt.arena.numels[i]
        step = (opt.arena.data[o:o + n] - p0[o:o + n] * (1 - 0.02 * 1e-4)).double()
        rms = float(step.pow(2).mean().sqrt()) / (0.02 * opt._geometry(i)[5])
        K, rest = opt._geometry(i)[:2]  # |O|_F^2 <= min(K, rest) * 1.15^2: singular values in the band
        assert 0.0 < rms * (max(K, rest) ** 0.5) < 1.3, (i, K, rest, rms)  # changed, and no larger
