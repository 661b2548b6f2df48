"""The wide classifier head (csrc/kernels/linear_wide.hip: 16 < J <= 128 on MFMA), exact and
bound mode of tests/exactness.py, and VGG-11 with 100 classes against the CPU oracles.

Roundings of the bound-mode tests, counted from the kernels:

| quantity                         | roundings                                                   |
|----------------------------------|-------------------------------------------------------------|
| logit = x . bf16(W) + b          | one bf16 rounding of each W element (b T), then F products  |
|                                  | and additions in any order plus the bias: (F + 1) u T       |
| dx = bf16(g (bf16(dl) . bf16(W)))| both operands rounded: (2 b + b^2) T; JP products and       |
|                                  | additions and the scale by g: JP u T; one bf16 store        |
| dW += g (bf16(dl)^T . x)         | dl rounded (x is bf16 already): b T; B products and         |
|                                  | additions, the scale, the add: (B + 2) u T                  |
| db += g sum_b dl                 | fp32 dl: B additions, the scale, the add: (B + 2) u T       |
"""
import copy
import functools

import pytest
import torch

from exactness import BF16_EPS as b_, FP32_EPS as u_, assert_exact, assert_within, dot_bound, \
    gauss_bf16, int_tensor
from test_gpu_elementwise import _head_inputs, ce_bounds
from test_gpu_model import _emulated_vgg_forward, rel
from test_gpu_soft_targets import E_LAM, soft_ce_bounds

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
SHAPES = [(B, Fi, J) for J in (17, 100, 128) for B in (3, 33) for Fi in (32, 96, 512)]


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def _fwd(nat, x, W, bias, labels, logits=None, dl=None, correct=None, soft=None):
    """One head launch on CPU operands; returns the loss accumulator."""
    from ddp_amd.ops.common import ptr, stream_handle
    B, Fi = x.shape
    loss = torch.zeros((), device=DEV)
    dev = [x.to(BF16).to(DEV), W.to(DEV), bias.to(DEV), None if labels is None else labels.to(DEV)]
    nat.linear_ce_fwd(ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), B, Fi, W.shape[0],
                      ptr(logits), ptr(dl), ptr(loss), ptr(correct), stream_handle(),
                      **({"soft": soft} if soft is not None else {}))
    torch.cuda.synchronize()
    return loss


def _bwd(nat, dl, x, W, gs, dx, dW, db):
    from ddp_amd.ops.common import ptr, stream_handle
    B, Fi = x.shape
    g = torch.tensor([gs], device=DEV)
    dev = [dl.to(DEV), x.to(BF16).to(DEV), W.to(DEV)]
    nat.linear_bwd(ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), B, Fi, W.shape[0], ptr(g), ptr(dx),
                   ptr(dW), ptr(db), stream_handle())
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,Fi,J", SHAPES)
def test_wide_forward_exact(native_ext, B, Fi, J):
    """Integer operands: logits bit for bit, and ``correct`` by the first fp64 maximum. Class
    J - 1 duplicates class 5, whose weights are row 0's features, so row 0 ties its two largest
    logits and its label J - 1 is a miss."""
    x = int_tensor((B, Fi), -4, 4, 10 + J)
    W, bias = int_tensor((J, Fi), -4, 4, 11 + Fi), int_tensor((J,), -4, 4, 12 + B)
    W[5] = x[0]
    W[J - 1], bias[J - 1] = W[5], bias[5]
    ref = x.double() @ W.double().t() + bias.double()
    absref = x.double().abs() @ W.double().abs().t() + bias.double().abs()
    assert float(absref.max()) <= 8208
    first = torch.tensor([int(torch.nonzero(r == r.max())[0]) for r in ref])
    labels = torch.where(torch.arange(B) % 2 == 1, first, int_tensor((B,), 0, J - 1, 13).long())
    labels[0] = J - 1
    assert int(first[0]) == 5 and ref[0, 5] == ref[0, J - 1]
    logits = _nan(B, J)
    _fwd(native_ext, x, W, bias, None, logits=logits)
    assert_exact(logits, ref, absref, ("b", "j"), what="logits")
    correct = torch.zeros((), dtype=torch.int32, device=DEV)
    _fwd(native_ext, x, W, bias, labels, correct=correct)
    assert int(correct) == int((first == labels).sum())


@pytest.mark.parametrize("B,Fi,J", SHAPES)
def test_wide_backward_exact(native_ext, B, Fi, J):
    """Integer dl, x, W and g = 0.5 onto pre-filled gradients: dx = bf16(0.5 dl W), dW and db bit
    for bit; without dx / without db the other outputs are the same and nothing else is written."""
    dl = int_tensor((B, J), -4, 4, 20 + Fi)
    x, W = int_tensor((B, Fi), -4, 4, 21 + J), int_tensor((J, Fi), -4, 4, 22 + B)
    pW, pb = int_tensor((J, Fi), -3, 3, 23), int_tensor((J,), -3, 3, 24)
    d64, x64, W64 = dl.double(), x.double(), W.double()
    refs = {"dx": (0.5 * d64 @ W64, d64.abs() @ W64.abs(), ("b", "f")),
            "dW": (pW.double() + 0.5 * d64.t() @ x64, 3 + d64.abs().t() @ x64.abs(), ("j", "f")),
            "db": (pb.double() + 0.5 * d64.sum(0), 3 + d64.abs().sum(0), ("j",))}
    for skip in (None, "dx", "db"):
        got = {"dx": _nan(B, Fi, dtype=BF16), "dW": pW.to(DEV), "db": pb.to(DEV)}
        _bwd(native_ext, dl, x, W, 0.5, *[None if k == skip else got[k] for k in ("dx", "dW", "db")])
        if skip == "dx":
            assert bool(torch.isnan(got.pop("dx").float()).all())
        if skip == "db":
            assert torch.equal(got.pop("db").cpu(), pb)
        for k, t in got.items():
            assert_exact(t, *refs[k][:2], refs[k][2], what=f"{k} (without {skip})", unit=0.5)


@functools.lru_cache(maxsize=None)
def _gauss_case(B, Fi, J):
    """Gaussian operands, their fp64 logits and the logit bound (module docstring)."""
    _, _, _, W, bias, labels = _head_inputs(B, Fi, J, 800 + Fi + J)
    x = gauss_bf16((B, Fi), 801 + B)
    Wd, bd = W.double(), bias.double()
    logits = x.double() @ Wd.t() + bd
    T = x.double().abs() @ Wd.abs().t() + bd.abs()
    return x, W, bias, labels, logits, b_ * T + (1 + b_) * (Fi + 1) * u_ * T


@pytest.mark.parametrize("B,Fi,J", SHAPES)
def test_wide_forward_backward_bounds(native_ext, B, Fi, J):
    """Gaussian operands: logits, loss and every dlogits element within their bounds; then the
    backward on the dlogits the forward produced, g = 2: dx, dW and db per element."""
    x, W, bias, labels, logits64, lb = _gauss_case(B, Fi, J)
    assert int(labels.min()) == 0 and int(labels.max()) == J - 1
    logits, dl = _nan(B, J), _nan(B, J)
    loss = _fwd(native_ext, x, W, bias, labels, logits=logits, dl=dl)
    print("logits", assert_within(logits, logits64, lb, ("b", "j"), what="logits"))
    want, loss_bound, d, d_bound = ce_bounds(logits64, labels, lb, J, 0)
    print("loss", assert_within(loss.cpu().double().view(1), want.view(1), loss_bound.view(1),
                                what="loss"))
    print("dlogits", assert_within(dl, d, d_bound, ("b", "j"), what="dlogits"))
    gs, JP = 2.0, -(-J // 16) * 16
    dx, dW, db = _nan(B, Fi, dtype=BF16), torch.zeros(J, Fi, device=DEV), torch.zeros(J, device=DEV)
    _bwd(native_ext, dl.cpu(), x, W, gs, dx, dW, db)
    d64, x64, W64 = dl.double().cpu() * gs, x.double(), W.double()
    ref, T = d64 @ W64, d64.abs() @ W64.abs()
    bound = b_ * ref.abs() + (1 + b_) * (dot_bound(ref, T, JP, 0) + (2 * b_ + b_ * b_) * T)
    print("dx", assert_within(dx, ref, bound, ("b", "f"), what="dx"))
    ref, T = d64.t() @ x64, d64.abs().t() @ x64.abs()
    print("dW", assert_within(dW, ref, b_ * T + (1 + b_) * (B + 2) * u_ * T, ("j", "f"), what="dW"))
    print("db", assert_within(db, d64.sum(0), (B + 2) * u_ * d64.abs().sum(0), ("j",), what="db"))


@pytest.mark.parametrize("E,lam", E_LAM)
@pytest.mark.parametrize("B,Fi,J", [s for s in SHAPES if s[2] != 128])
def test_wide_forward_soft(native_ext, B, Fi, J, E, lam):
    """Soft targets, partner labels = the labels reversed: loss and dlogits per element."""
    from ddp_amd.ops.common import ptr
    x, W, bias, labels, logits64, lb = _gauss_case(B, Fi, J)
    yb = labels.flip(0).contiguous()
    ybd, lam_d = yb.to(DEV), torch.tensor([lam], dtype=torch.float32, device=DEV)
    dl = _nan(B, J)
    loss = _fwd(native_ext, x, W, bias, labels, dl=dl, soft=(E, ptr(ybd), ptr(lam_d)))
    want, loss_bound, d, d_bound = soft_ce_bounds(logits64, labels, yb, E, lam, lb, J, 0)
    print("loss", assert_within(loss.cpu().double().view(1), want.view(1), loss_bound.view(1),
                                what="loss"))
    print("dlogits", assert_within(dl, d, d_bound, ("b", "j"), what="dlogits"))


@pytest.mark.parametrize("J", [17, 100])
def test_wide_soft_neutral_is_plain(native_ext, J):
    """E = 0, lam = 1 through the soft instantiation: dlogits torch.equal to the plain call's."""
    from ddp_amd.ops.common import ptr
    x, W, bias, labels, _, _ = _gauss_case(33, 96, J)
    ybd, one = labels.flip(0).to(DEV), torch.ones(1, device=DEV)
    dl0, dl1 = _nan(33, J), _nan(33, J)
    _fwd(native_ext, x, W, bias, labels, dl=dl0)
    _fwd(native_ext, x, W, bias, labels, dl=dl1, soft=(0.0, ptr(ybd), ptr(one)))
    assert torch.equal(dl1, dl0)


@pytest.mark.parametrize("route", ["logits", "forward_loss"])
def test_vgg11_100_classes_matches_cpu_oracle(native_ext, route):
    """test_vgg11_forward_backward_matches_cpu_oracle with a 100-way head, its constants, through
    model(x) + CrossEntropyLoss and through forward_loss; forward_metrics counts the argmax hits."""
    from ddp_amd.models import VGG11
    from ddp_amd.engine import CrossEntropyLoss
    from ddp_amd.optim import FusedSGD
    torch.manual_seed(1)
    cpu = VGG11(num_classes=100)
    emu, gpu = copy.deepcopy(cpu), copy.deepcopy(cpu).cuda()
    FusedSGD(gpu.parameters(), lr=0.1).zero_grad()
    x = torch.randn(32, 3, 32, 32).to(BF16).float()
    y = torch.randint(0, 100, (32,))
    crit = CrossEntropyLoss()
    lc = crit(cpu(x), y)
    le = crit(_emulated_vgg_forward(emu, x), y)
    le.backward()
    xg, yg = x.cuda(), y.cuda()
    lg = crit(gpu(xg), yg) if route == "logits" else gpu.forward_loss(xg, yg)
    lg.backward()
    torch.cuda.synchronize()
    assert abs(float(lg) - float(lc)) < 0.05 * max(1.0, abs(float(lc)))
    assert abs(float(lg) - float(le)) < 1e-2 * max(1.0, abs(float(le)))
    for (n, pe), pg in zip(emu.named_parameters(), gpu.parameters()):
        g, e = pg.grad.cpu().reshape(-1), pe.grad.reshape(-1)
        if n.startswith("layers.") and n.endswith("bias") and \
                isinstance(emu.layers[int(n.split(".")[1])], torch.nn.Conv2d):
            continue  # analytically zero (the oracle test bounds the noise)
        assert float(torch.dot(g, e) / (g.norm() * e.norm() + 1e-20)) >= 0.95, n
        if n in ("fc1.weight", "fc1.bias", "layers.26.weight", "layers.26.bias"):
            assert rel(g, e) < 0.03, (n, rel(g, e))
    hits = torch.zeros((), dtype=torch.int32, device=DEV)
    gpu.forward_metrics(xg, yg, torch.zeros((), device=DEV), hits)
    with torch.no_grad():
        assert int(hits) == int((gpu(xg).argmax(1) == yg).sum())


def test_head_refuses_129_outputs(native_ext):
    from ddp_amd.ops.layers import linear_cross_entropy
    lin = torch.nn.Linear(512, 129).to(DEV)
    with pytest.raises(ValueError, match="128"):
        linear_cross_entropy(torch.zeros(4, 512, device=DEV, dtype=BF16), lin,
                             torch.zeros(4, dtype=torch.int64, device=DEV))
