"""Ghost BatchNorm + ReLU (+ 2x2 pool) kernels (ghost_bn.hip): every element of y, the (mu, is)
table, dz, dgamma and dbeta against F.batch_norm per interleaved group -> relu -> max_pool2d and
their autograd in fp64 (tests/exactness.py assert_within); the bitwise split invariance the
feature exists for; the refusals; the captured VGG-11 step.

Bounds, counted from ghost_bn.hip (u = 2**-24 per fp32 rounding, b = 2**-8 per bf16 store; a sum
of k terms in any order counts k roundings of the sum of magnitudes). Per (group, channel): m
elements in K chunks of at most nb, zmax = max |z|, d = z - mu, q = sum d^2. By Cauchy-Schwarz
sum |d| and sum_k w_k |delta_k| (w_k the Chan weight) are both at most sqrt(m q).

| quantity                                    | roundings                                     | term |
|---------------------------------------------|-----------------------------------------------|------|
| mean_b = (sum z) / n_b                      | nb on the sum, 1                              |      |
| mu: mean += delta * (n_b / n_t), K times    | delta, quotient, fma, both operands' means: 5 | dmu  |
|   dmu = (nb + 1 + 5 K) u zmax               |                                               |      |
| M2_b = sum fma(d_b, d_b), d_b = z - mean_b  | the centre's (nb + 1) u zmax; nb + 3          |      |
| M2 = (M2 + M2_b) + delta^2 * (n n_b / n_t)  | delta: 2 dmu + u; 5 on the term; 2 K sums     | dq   |
|   dq = sqrt(m q) (2 (nb + 1) u zmax + 4 dmu) + (nb + 10 + 2 K) u q                          |      |
| var = M2 / m                                | 1                                             | dv   |
| is = rsqrtf(var + eps)                      | (dv / (var + eps) + 1) / 2; v_rsq 1 ulp: 2    | ris  |
| xhat = (z - mu) * is                        | dmu, 1 sub, ris, 1 product                    | dxh  |
| pre = fma(xhat, gamma, beta)                | |gamma| dxh + 1                               | dy   |
| S1 = sum dyb (chunk sums, then K adds)      | nb + K                                        | dS1  |
| S2 = sum fma(dyb, xhat)                     | dxh per term; nb + K + 1                      | dS2  |
| k = S * inv_m, inv_m = 1 / m                | 2                                             | dk   |
| dz = (gamma * is) * fma(-xhat, k2, dyb - k1)| sub, fma; scale: ris + 1, product; bf16 store | ddz  |
| dgamma, dbeta += sum_g S_g                  | ngroups + 1                                   |      |

An undecidable element (test_gpu_elementwise.bn_undecidable) may gain or lose its window's
gradient: slack ``mv`` in the sums; such elements are excluded from dz, at most 2 % of a case."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from exactness import BF16_EPS as b_, FP32_EPS as u_, assert_within, int_tensor
from test_gpu_elementwise import (BF16, DEV, EPS, NHWC, _cv, _dev_nhwc, _nhwc, bn_out_bound,
                                  bn_undecidable)
from test_gpu_group_norm import _inputs

pytestmark = pytest.mark.gpu

CASES = [(4, 2, 2, 64, 2, True), (5, 4, 4, 64, 2, False), (3, 16, 16, 32, 3, True),
         (6, 5, 3, 40, 4, False), (2, 32, 32, 8, 1, True), (9, 8, 8, 256, 4, False),
         (64, 2, 2, 512, 32, True)]


def _chunking(H, W, C, pool, cnt):
    """(elements per channel of a full chunk, chunks) of a group of ``cnt`` images: the plan of
    ghost_bn.hip (the widest slab of 8-channel lanes for which one image fits a chunk)."""
    U, per = (H * W // 4, 1) if pool else (H * W, 4)
    CL = next((cl for cl in range(min(64, C // 8), 1, -1)
               if C // 8 % cl == 0 and U <= 256 // cl * per), 1)
    cap = 256 // CL * per
    return min(cap, cnt * U) * (4 if pool else 1), -(-cnt * U // cap)


def gbn_reference(z, gamma, beta, dout, G, pool, init):
    """fp64 reference (F.batch_norm per group n % ngroups -> relu -> max_pool2d, autograd) and the
    bounds of the table in the module docstring. ``init`` [2][C]: what dgamma / dbeta hold."""
    N, C, H, W = z.shape
    ng = -(-N // G)
    cnts = [len(range(g, N, ng)) for g in range(ng)]
    m = torch.tensor([c * H * W for c in cnts], dtype=torch.float64).view(ng, 1)
    nb, K = (torch.tensor(v, dtype=torch.float64).view(ng, 1)
             for v in zip(*[_chunking(H, W, C, pool, c) for c in cnts]))
    grp = lambda v: torch.stack([v[g::ng].sum((0, 2, 3)) for g in range(ng)])  # [ng][C]
    bc = lambda t: t[torch.arange(N) % ng][:, :, None, None]
    zl = z.clone().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = torch.empty_like(z)
    for g in range(ng):
        y[g::ng] = F.batch_norm(zl[g::ng], None, None, g64, b64, True, 0.0, EPS)
    y.retain_grad()
    a = F.relu(y)
    (F.max_pool2d(a, 2, 2) if pool else a).backward(dout)
    dyb, dz, y = y.grad, zl.grad, y.detach()
    # ---- forward
    mu = grp(z) / m
    d = z - bc(mu)
    q = grp(d * d)
    var = q / m
    ve = var + EPS
    is_ = ve.rsqrt()
    zmax = torch.stack([z[g::ng].abs().amax((0, 2, 3)) for g in range(ng)])
    dmu = (nb + 1 + 5 * K) * u_ * zmax
    dq = (m * q).sqrt() * (2 * (nb + 1) * u_ * zmax + 4 * dmu) + (nb + 10 + 2 * K) * u_ * q
    dv = dq / m + u_ * var
    ris = 0.5 * (dv / ve + u_) + 2 * u_
    xh = d * bc(is_)
    dxh = bc(is_) * (bc(dmu) + u_ * d.abs()) + xh.abs() * bc(ris + u_)
    ga = _cv(gamma.double())
    t = dict(y=y, dy=ga.abs() * dxh + u_ * y.abs(), z=z, gamma=gamma.double())
    out, out_bound = bn_out_bound(t, True, pool)
    ex = bn_undecidable(t, True, pool)
    # ---- backward
    up = (lambda v: v.repeat_interleave(2, -2).repeat_interleave(2, -1)) if pool else (lambda v: v)
    xm = up(F.max_pool2d(xh.abs(), 2, 2)) if pool else xh.abs()
    mv = torch.where(ex, up(dout.abs()), torch.zeros_like(z))
    S1, S2 = grp(dyb), grp(dyb * xh)
    dS1 = (nb + K) * u_ * grp(dyb.abs()) + grp(mv)
    dS2 = grp(dyb.abs() * dxh) + (nb + K + 1) * u_ * grp((dyb * xh).abs()) + grp(mv * 2 * xm)
    k1, k2 = S1 / m, S2 / m
    dk1, dk2 = dS1 / m + 2 * u_ * k1.abs(), dS2 / m + 2 * u_ * k2.abs()
    inner = dyb - bc(k1) - xh * bc(k2)
    din = (bc(dk1) + bc(k2.abs()) * dxh + xh.abs() * bc(dk2)
           + u_ * ((dyb - bc(k1)).abs() + inner.abs()))
    ddz = (ga * bc(is_)).abs() * din + dz.abs() * bc(ris + 2 * u_)
    r = (ng + 1) * u_
    return dict(
        out=out, out_bound=out_bound, ex=ex, dz=dz, dz_bound=b_ * dz.abs() + (1 + b_) * ddz,
        table=torch.stack([mu, is_], 1), table_bound=torch.stack([dmu, ris * is_], 1),
        sums=init.double() + torch.stack([g64.grad, b64.grad]),
        sums_bound=torch.stack([dS2.sum(0) + r * (S2.abs().sum(0) + init[0].abs()),
                                dS1.sum(0) + r * (S1.abs().sum(0) + init[1].abs())]))


def _buffers(N, H, W, C, G, pool):
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    nan = lambda *s, dt=BF16: torch.full(s, float("nan"), device=DEV, dtype=dt)
    return nan(N, Ho, Wo, C), nan(-(-N // G), 2, C, dt=torch.float32), nan(N, H, W, C)


def _fwd(nat, shape, zn, gd, bd, y, table):
    from ddp_amd.ops.common import ptr, stream_handle, workspace
    N, H, W, C, G, pool = shape
    ws = workspace(torch.device(DEV))
    nat.gbn_act_fwd(N, H, W, C, G, int(pool), 1, EPS, ptr(zn), ptr(gd), ptr(bd), ptr(y),
                    ptr(table), ptr(ws), ws.numel(), stream_handle())


def _bwd(nat, shape, zn, gd, bd, table, doutn, dz, sums):
    from ddp_amd.ops.common import ptr, stream_handle, workspace
    N, H, W, C, G, pool = shape
    ws = workspace(torch.device(DEV))
    nat.gbn_act_bwd(N, H, W, C, G, int(pool), 1, EPS, ptr(zn), ptr(gd), ptr(bd), ptr(table),
                    ptr(doutn), ptr(dz), ptr(sums[0]), ptr(sums[1]), ptr(ws), ws.numel(),
                    stream_handle())
    torch.cuda.synchronize()


def _run(nat, z, gamma, beta, dout, G, pool, sums):
    """y, table, dz of the kernels (NaN-filled before); dgamma / dbeta accumulate into ``sums``."""
    N, C, H, W = z.shape
    shape = (N, H, W, C, G, pool)
    y, table, dz = _buffers(*shape)
    dev = (_dev_nhwc(z), gamma.to(DEV), beta.to(DEV))
    _fwd(nat, shape, *dev, y, table)
    _bwd(nat, shape, *dev, table, _dev_nhwc(dout), dz, sums)
    return y, table, dz


@pytest.mark.parametrize("N,H,W,C,G,pool", CASES)
def test_gbn_per_element(native_ext, N, H, W, C, G, pool):
    z, gamma, beta, dout = _inputs(N, H, W, C, pool, 700 + C + H)
    init = int_tensor((2, C), 1, 7, 77)
    r = gbn_reference(z, gamma, beta, dout, G, pool, init)
    sums = init.to(DEV)
    y, table, dz = _run(native_ext, z, gamma, beta, dout, G, pool, sums)
    print("y", assert_within(y, _nhwc(r["out"]), _nhwc(r["out_bound"]), NHWC, what="y"))
    print("table", assert_within(table, r["table"], r["table_bound"], ("g", "mu|is", "c"),
                                 what="(mu, is) table"))
    print("dz", assert_within(dz, _nhwc(r["dz"]), _nhwc(r["dz_bound"]), NHWC,
                              exclude=_nhwc(r["ex"]), max_excluded=0.02, what="dz"))
    print("sums", assert_within(sums, r["sums"], r["sums_bound"], ("dgamma|dbeta", "c"),
                                what="dgamma / dbeta"))


@pytest.mark.parametrize("H,C,pool", [(4, 64, True), (16, 32, False)])
def test_gbn_split_invariance(native_ext, H, C, pool):
    """Two ranks of 4 see the bits one rank of 8 does: y[g::2] and dz[g::2] of N = 8, ghost 4
    equal a separate N = 4, ghost 4 call on z[g::2], dy[g::2] (the chunk plan ignores ngroups)."""
    z, gamma, beta, dout = _inputs(8, H, H, C, pool, 900 + H)
    sums = torch.zeros(2, C, device=DEV)
    y, table, dz = _run(native_ext, z, gamma, beta, dout, 4, pool, sums)
    for g in range(2):
        yh, th, dzh = _run(native_ext, z[g::2], gamma, beta, dout[g::2], 4, pool, sums.clone())
        assert torch.equal(y[g::2], yh) and torch.equal(dz[g::2], dzh)
        assert torch.equal(table[g], th[0])
    assert not bool(torch.isnan(y.float()).any() | torch.isnan(dz.float()).any())


@pytest.mark.parametrize("N,H,W,C,G,pool", [(2, 4, 4, 12, 2, False), (2, 5, 4, 64, 2, True)])
def test_gbn_refusals(native_ext, N, H, W, C, G, pool):
    from ddp_amd.models import GhostBatchNorm2d
    from ddp_amd.ops.common import workspace
    from ddp_amd.ops.layers import ConvGhostBNActSpec, conv_gbn_act
    assert not native_ext.gbn_ok(N, H, W, C, G, int(pool), workspace(torch.device(DEV)).numel())
    shape = (N, H, W, C, G, pool)
    y, table, dz = _buffers(*shape)
    zn = torch.ones(N, H, W, C, device=DEV, dtype=BF16)
    sums = torch.ones(2, C, device=DEV)
    with pytest.raises(RuntimeError, match="invalid arguments"):
        _fwd(native_ext, shape, zn, sums[0], sums[1], y, table)
    with pytest.raises(RuntimeError, match="invalid arguments"):
        _bwd(native_ext, shape, zn, sums[0], sums[1], table, torch.ones_like(y), dz, sums)
    torch.cuda.synchronize()
    for t in (y, table, dz):
        assert bool(torch.isnan(t.float()).all())
    assert bool((sums == 1).all())
    with pytest.raises(ValueError, match="multiple of 8"):
        conv = nn.Conv2d(8, C, 3, padding=1).to(DEV)
        spec = ConvGhostBNActSpec(conv, GhostBatchNorm2d(C, G).to(DEV), pool=pool)
        conv_gbn_act(torch.ones(N, H, W, 8, device=DEV, dtype=BF16), spec)


def test_ghost_vgg_captured_replay_equals_eager(native_ext):
    from ddp_amd.models import VGG11
    from ddp_amd.engine import CrossEntropyLoss, TrainStep
    from ddp_amd.optim import FusedSGD
    from ddp_amd.data import SyntheticCIFAR10, DeviceLoader
    torch.manual_seed(5)
    m = VGG11(norm="ghost", ghost_batch=4).cuda()
    opt = FusedSGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    ld = DeviceLoader(SyntheticCIFAR10(True, n=64), 8, "cuda")
    st = TrainStep(m, opt, CrossEntropyLoss(), ld, use_graph=True)
    st.warmup(2)
    st.capture()
    st.pop_loss()
    snap = (opt.arena.data.clone(), opt.momentum_buffer.clone(), ld.cursor.clone())
    st._body()  # eager
    eager = st.pop_loss()
    opt.arena.data.copy_(snap[0]); opt.momentum_buffer.copy_(snap[1]); ld.cursor.copy_(snap[2])
    for sp in m.fused_plan():
        sp._packed_version = None
        sp.maybe_pack()
    st.step()  # graph replay of the same step
    first = st.pop_loss()
    assert abs(first - eager) < 5e-3 * max(1.0, abs(eager)), (first, eager)
    st.step()
    second = st.pop_loss()
    assert second == second and abs(second) < 1e4 and second != first, (first, second)
