"""GroupNorm + ReLU (+ 2x2 pool) kernels (group_norm.hip): every element of y, dz, the (mu, is)
table, dgamma, dbeta and dbias against F.group_norm -> relu -> max_pool2d and their autograd in
fp64 (tests/exactness.py assert_within); the refusals; a two-block conv_gn_act stack against the
bf16-emulating CPU oracle; the captured VGG-11 step.

Bounds, counted from group_norm.hip (u = 2**-24 per fp32 rounding, b = 2**-8 per bf16 store; a
sum of k terms in any order counts k roundings of the sum of magnitudes; m = Cg * H * W elements
per group, M = N * H * W per channel):

| quantity                                     | roundings                                  | term     |
|----------------------------------------------|--------------------------------------------|----------|
| mu = (sum z) * inv_m                         | m on the sum; fl(1 / m), product: 2        | dmu      |
| q = sum fma(d, d, q), d = z - mu             | d: dmu + 1; m on the sum                   | dq       |
| var = q * inv_m                              | 2                                          | dv       |
| is = rsqrtf(var + eps)                       | (dv / (var + eps) + 1) / 2; v_rsq 1 ulp: 2 | ris      |
| xhat = (z - mu) * is                         | dmu, 1 sub, ris, 1 product                 | dxh      |
| pre = fma(xhat, gamma, beta)                 | |gamma| dxh + 1                            | dy       |
| A = sum fma(gamma, sum dyb)                  | m + 2                                      | dA       |
| B = sum fma(gamma, sum fma(dyb, xhat))       | dxh per term; m + 2                        | dB       |
| kA = A * inv_m, kB = B * inv_m               | 2 each                                     | dkA, dkB |
| dz = is * fma(-xhat, kB, dyb * gamma - kA)   | product, sub, fma: 3; ris + 1; bf16 store  | ddz      |
| dgamma, dbeta, dbias (fp32 dz) += over M     | M (lane, LDS, partials, finish) + 2 (+=)   |          |

is's relative error multiplies |(z - mu) * is|. An undecidable element (the rule of
test_gpu_elementwise.bn_undecidable) may gain or lose its window's gradient: slack ``mv``."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from exactness import BF16_EPS as b_, FP32_EPS as u_, assert_within, gauss_bf16, int_tensor
from test_gpu_elementwise import (BF16, DEV, EPS, NHWC, _cv, _dev_nhwc, _nhwc, bn_out_bound,
                                  bn_undecidable)
from test_gpu_model import _Q, _QW, rel

pytestmark = pytest.mark.gpu

CASES = [(3, 4, 4, 64, 32, True), (3, 16, 16, 32, 32, False), (2, 5, 3, 40, 5, False),
         (2, 2, 2, 512, 32, True), (2, 6, 10, 128, 8, True), (2, 1, 1, 128, 2, False),
         (5, 8, 8, 256, 32, False), (2, 32, 32, 64, 32, True)]


def _inputs(N, H, W, C, pool, seed):
    z = gauss_bf16((N, C, H, W), seed, 2.0, 0.5).double()
    g = torch.Generator().manual_seed(seed + 1)
    gamma = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
    gamma[2] = 0.0
    assert bool((gamma > 0).any()) and bool((gamma < 0).any())
    beta = torch.randn(C, generator=g) * 0.1
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    return z, gamma.float(), beta.float(), gauss_bf16((N, C, Ho, Wo), seed + 2).double()


def gn_reference(z, gamma, beta, dout, G, pool, init):
    """fp64 reference (F.group_norm -> relu -> max_pool2d, autograd) and the bounds of the table
    in the module docstring. ``init`` [3][C]: what dgamma / dbeta / dbias hold before."""
    N, C, H, W = z.shape
    m, M, sh = C // G * H * W, N * H * W, z.shape
    grp = lambda v: v.reshape(N, G, -1).sum(-1)
    bc = lambda t: t.reshape(N, G, 1, 1, 1).expand(N, G, C // G, H, W).reshape(sh)
    sm = lambda v: v.sum((0, 2, 3))
    zl = z.clone().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.group_norm(zl, G, g64, b64, EPS)
    y.retain_grad()
    a = F.relu(y)
    (F.max_pool2d(a, 2, 2) if pool else a).backward(dout)
    dyb, dz, y = y.grad, zl.grad, y.detach()
    # ---- forward
    mu = grp(z) / m
    d = z - bc(mu)
    var = grp(d * d) / m
    ve = var + EPS
    is_ = ve.rsqrt()
    dmu = u_ * grp(z.abs()) + 2 * u_ * mu.abs()
    dq = grp(2 * d.abs() * (bc(dmu) + u_ * d.abs())) + m * u_ * grp(d * d)
    dv = dq / m + 2 * u_ * var
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
    dxhat, gd = ga * dyb, (ga * dyb).abs()
    A, B = grp(dxhat), grp(dxhat * xh)
    dA = (m + 2) * u_ * grp(gd) + grp(ga.abs() * mv)
    dB = grp(gd * dxh) + (m + 2) * u_ * grp(gd * xh.abs()) + grp(ga.abs() * mv * 2 * xm)
    kA, kB = A / m, B / m
    dkA, dkB = dA / m + 2 * u_ * kA.abs(), dB / m + 2 * u_ * kB.abs()
    inner = dxhat - bc(kA) - xh * bc(kB)
    din = (bc(dkA) + bc(kB.abs()) * dxh + xh.abs() * bc(dkB)
           + u_ * (gd + (dxhat - bc(kA)).abs() + inner.abs()))
    ddz = bc(is_) * din + dz.abs() * bc(ris + u_)
    r = (M + 2) * u_
    return dict(
        out=out, out_bound=out_bound, ex=ex, dz=dz, dz_bound=b_ * dz.abs() + (1 + b_) * ddz,
        table=torch.stack([mu, is_], -1), table_bound=torch.stack([dmu, ris * is_], -1),
        sums=init.double() + torch.stack([g64.grad, b64.grad, sm(dz)]),
        sums_bound=torch.stack([
            sm(dyb.abs() * dxh + mv * 2 * xm) + r * (sm((dyb * xh).abs()) + init[0].abs()),
            sm(mv) + r * (sm(dyb.abs()) + init[1].abs()),
            sm(ddz + bc(is_) * ga.abs() * mv) + r * (sm(dz.abs()) + init[2].abs())]))


def _buffers(N, H, W, C, G, pool):
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    nan = lambda *s, dt=BF16: torch.full(s, float("nan"), device=DEV, dtype=dt)
    return nan(N, Ho, Wo, C), nan(N, G, 2, dt=torch.float32), nan(N, H, W, C)


def _fwd(nat, shape, zn, gd, bd, y, table):
    from ddp_amd.ops.common import ptr, stream_handle
    N, H, W, C, G, pool = shape
    nat.gn_act_fwd(N, H, W, C, G, int(pool), 1, EPS, ptr(zn), ptr(gd), ptr(bd), ptr(y), ptr(table),
                   stream_handle())


def _bwd(nat, shape, zn, gd, bd, table, doutn, dz, sums, with_bias=True):
    from ddp_amd.ops.common import ptr, stream_handle, workspace
    N, H, W, C, G, pool = shape
    ws = workspace(torch.device(DEV))
    nat.gn_act_bwd(N, H, W, C, G, int(pool), 1, EPS, ptr(zn), ptr(gd), ptr(bd), ptr(table),
                   ptr(doutn), ptr(dz), ptr(sums[0]), ptr(sums[1]),
                   ptr(sums[2]) if with_bias else 0, ptr(ws), ws.numel(), stream_handle())
    torch.cuda.synchronize()


@pytest.mark.parametrize("N,H,W,C,G,pool", CASES)
def test_gn_act_per_element(native_ext, N, H, W, C, G, pool):
    z, gamma, beta, dout = _inputs(N, H, W, C, pool, 500 + C + H)
    init = int_tensor((3, C), 1, 7, 77)
    r = gn_reference(z, gamma, beta, dout, G, pool, init)
    y, table, dz = _buffers(N, H, W, C, G, pool)
    sums, shape = init.to(DEV), (N, H, W, C, G, pool)
    dev = (_dev_nhwc(z), gamma.to(DEV), beta.to(DEV))
    _fwd(native_ext, shape, *dev, y, table)
    _bwd(native_ext, shape, *dev, table, _dev_nhwc(dout), dz, sums)
    print("y", assert_within(y, _nhwc(r["out"]), _nhwc(r["out_bound"]), NHWC, what="y"))
    print("table", assert_within(table, r["table"], r["table_bound"], ("n", "g", "mu|is"),
                                 what="(mu, is) table"))
    print("dz", assert_within(dz, _nhwc(r["dz"]), _nhwc(r["dz_bound"]), NHWC,
                              exclude=_nhwc(r["ex"]), what="dz"))
    print("sums", assert_within(sums, r["sums"], r["sums_bound"], ("dgamma|dbeta|dbias", "c"),
                                what="dgamma / dbeta / dbias"))
    # a null dbias skips the third sum and changes nothing else
    s2 = init.to(DEV)
    _bwd(native_ext, shape, *dev, table, _dev_nhwc(dout), dz, s2, with_bias=False)
    assert torch.equal(s2[:2], sums[:2]) and torch.equal(s2[2].cpu(), init[2])


@pytest.mark.parametrize("N,H,W,C,G,pool", [
    (2, 4, 4, 24, 8, False),     # Cg = 3
    (2, 2, 2, 256, 2, False),    # Cg = 128
    (2, 4, 4, 12, 3, False),     # C = 12
    (2, 5, 4, 64, 32, True),     # odd H with the pool
    (2, 34, 32, 64, 32, False),  # 8 * 34 * 32 elements: over the resident budget of 8192
])
def test_gn_refusals(native_ext, N, H, W, C, G, pool):
    assert not native_ext.gn_ok(N, H, W, C, G, int(pool))
    y, table, dz = _buffers(N, H, W, C, G, pool)
    zn = torch.ones(N, H, W, C, device=DEV, dtype=BF16)
    sums = torch.ones(3, C, device=DEV)
    shape = (N, H, W, C, G, pool)
    with pytest.raises(RuntimeError, match="invalid arguments"):
        _fwd(native_ext, shape, zn, sums[0], sums[1], y, table)
    with pytest.raises(RuntimeError, match="invalid arguments"):
        _bwd(native_ext, shape, zn, sums[0], sums[1], table, torch.ones_like(y), dz, sums)
    for t in (y, table, dz):
        assert bool(torch.isnan(t.float()).all())
    assert bool((sums == 1).all())
    if C == 24:
        from ddp_amd.ops.layers import ConvGNActSpec
        with pytest.raises(ValueError, match="power of two"):
            ConvGNActSpec(nn.Conv2d(8, 24, 3, padding=1).to(DEV), nn.GroupNorm(8, 24).to(DEV))


def test_conv_gn_act_stack_matches_emulated_oracle(native_ext):
    """conv_gn_act twice (64 -> 64 pooled, 64 -> 128) against the CPU modules with bf16 rounding
    where the GPU path stores bf16; the conv BIAS gradient is compared like every other one (under
    BatchNorm it is analytically zero and the comparison would be vacuous)."""
    from ddp_amd.ops.layers import ConvGNActSpec, conv_gn_act
    torch.manual_seed(11)
    blocks = [(nn.Conv2d(64, 64, 3, padding=1), nn.GroupNorm(32, 64), True),
              (nn.Conv2d(64, 128, 3, padding=1), nn.GroupNorm(32, 128), False)]
    for _, gn, _ in blocks:
        gn.weight.data.uniform_(0.5, 1.5)
        gn.bias.data.normal_(0, 0.1)
    x = gauss_bf16((8, 64, 8, 8), 21)
    wgt = gauss_bf16((8, 128, 4, 4), 22)
    h = x
    for conv, gn, pool in blocks:
        zc = _Q.apply(F.conv2d(h, _QW.apply(conv.weight), conv.bias, 1, 1))
        yc = F.relu(F.group_norm(zc, gn.num_groups, gn.weight, gn.bias, gn.eps))
        h = _Q.apply(F.max_pool2d(yc, 2, 2) if pool else yc)
    (h * wgt).sum().backward()
    gblocks = [(copy.deepcopy(c).to(DEV), copy.deepcopy(g).to(DEV), p) for c, g, p in blocks]
    hg = _dev_nhwc(x)
    for (conv, gn, pool), hw in zip(gblocks, (8, 4)):
        hg = conv_gn_act(hg, ConvGNActSpec(conv, gn, pool=pool, hw=(hw, hw)))
    (hg.float() * _dev_nhwc(wgt).float()).sum().backward()
    torch.cuda.synchronize()
    assert rel(hg.detach().cpu(), _nhwc(h.detach())) < 1e-2
    for (conv, gn, _), (gc, gg, _) in zip(blocks, gblocks):
        for n, pc, pg in (("weight", conv.weight, gc.weight), ("bias", conv.bias, gc.bias),
                          ("gamma", gn.weight, gg.weight), ("beta", gn.bias, gg.bias)):
            e, g = pc.grad.reshape(-1), pg.grad.cpu().reshape(-1)
            assert float(e.norm()) > 0, n
            assert float(torch.dot(g, e) / (g.norm() * e.norm())) >= 0.95, n


def test_group_vgg_captured_replay_equals_eager(native_ext):
    from ddp_amd.models import VGG11
    from ddp_amd.engine import CrossEntropyLoss, TrainStep
    from ddp_amd.optim import FusedSGD
    from ddp_amd.data import SyntheticCIFAR10, DeviceLoader
    torch.manual_seed(5)
    m = VGG11(norm="group").cuda()
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
