"""Squeeze-and-Excitation kernels (se.hip): every element of the tables and outputs against an
fp64 reference that applies the kernel's store points (tests/exactness.py), the refusals, an SE
Bottleneck against its CPU module, and captured replays of a small SE-ResNet against eager steps.

Per-element inputs are integer-valued bf16 (|z|, |res| <= 4, |dy| <= 3): S, G1, G2 (at most 196
integers below 13) and dres are exact in fp32 in any order. The weights are bf16 numbers.

Bounds, counted from se.hip (u = 2**-24 per fp32 rounding, b = 2**-8 per bf16 store; a sum of k
terms counts k roundings of the sum of magnitudes; d(x) is the bound of x, M = N * HW):

| quantity                                          | roundings                                    |
|---------------------------------------------------|----------------------------------------------|
| mu = s1 / M; var = s2 / M - mu * mu               | 1; 1, 2 |mu| d(mu) + 1 on mu^2, 1            |
| is = rsqrtf(var + eps)                            | rel: d(var) / 2(var + eps) + 1 (add) + 2     |
| sc = gamma * is; sh = beta - mu * sc              | 1; product 1, d(mu), d(sc), sub 1            |
| m = fma(sc, S * inv_hw, sh)                       | inv_hw 1, product 1; d(sc), d(sh); fma 1     |
| h = max(t1, 0), t1 = bf16(m) . W1 + b1 (4 waves)  | b |m| + d(m) per operand; C + 3 on the sum   |
| t2 = bf16(h) . W2 + b2                            | b |h| + d(h) per operand; Cr + 3 on the sum  |
| s = 1 / (1 + expf(-t2))                           | s (1 - s) d(t2); expf 2, add 1, divide 1: 6  |
| v = fma(fma(sc, z, sh), s, res); y = bf16(max)    | d(sc), d(sh), 1; d(s), 1; b |y| on the store |
| ds = fma(sc, G2, sh * G1); dt2 = ds * (s (1 - s)) | d(sc), d(sh), 2; d(s), 2 on s (1 - s); 1     |
| dh = (bf16(dt2) . W2) [h > 0]                     | b |dt2| + d(dt2) per operand; C + 3          |
| dm = bf16(dh) . W1                                | b |dh| + d(dh) per operand; Cr + 3           |
| dW2 += dt2^T h; dW1 += dh^T m; db2; db1 (fp32)    | operand bounds; N + 2 on the sum (with +=)   |
| T1 = sum_n fma(s, G1, dm); T2 = .. dm (S inv_hw)  | d(s), d(dm), 1 (2 for T2) per term; N + 1    |
| dbeta += T1; dgamma += sxh = is * fma(-mu, T1, T2)| d(T1), d(T2), d(mu), 1; rel d(is) + 1; += 1  |
| k1 = T1 * inv_m; k2 = sxh * inv_m; xhat (below)   | 2 each; d(mu), sub 1, rel d(is) + 1          |
| du = fma(dy mask, s, dm * inv_hw)                 | d(s), d(dm) / HW + 2, 1                      |
| dz = bf16(sc * fma(-xhat, k2, du - k1))           | sub 1, fma 1, product 1; b |dz| on the store |

The reference rounds m, h, dt2, dh to bf16 where the kernel does; a kernel operand that lands on
the other side of a rounding boundary is covered by the b |x| term of the sum it enters. Elements
whose pre-ReLU value lies within its bound of 0 are undecidable (assert_within ``exclude``) and
lend their |dy| (|dy z|) to the bounds of G1 (G2) and of what follows; an fc1 output within its
bound of 0 is not allowed (checked on the reference)."""
import copy

import pytest
import torch

from exactness import BF16_EPS as b_, FP32_EPS as u_, assert_within, gauss_bf16, int_tensor

pytestmark = pytest.mark.gpu
DEV, BF16, EPS = "cuda", torch.bfloat16, 1e-5
CASES = [(1, 1, 1, 64, 16), (3, 2, 2, 256, 16), (17, 7, 7, 128, 16), (32, 14, 14, 512, 32),
         (2, 4, 4, 2048, 128)]


_rb = lambda x: x.to(BF16).double()  # noqa: E731  (a bf16 store point)


def se_reference(t, running):
    """fp64 values and bounds of every table and output; ``t``: the inputs (fp64 / fp32 CPU)."""
    z, res, dy = t["z"], t["res"], t["dy"]              # [N][HW][C]
    N, HW, C = z.shape
    M = N * HW
    W1, b1, W2, b2 = (t[k].double() for k in ("w1", "b1", "w2", "b2"))
    gamma, beta = t["gamma"].double(), t["beta"].double()
    if running:
        mu, var = t["rm"].double(), t["rv"].double()
        dmu = dvar = torch.zeros(C, dtype=torch.float64)
    else:
        # (a rounding counts only where its result is not an fp32 number: M = 1 is exact)
        rnd = lambda x, dep=0.0: u_ * x.abs() * ((x.float().double() != x) | (dep > 0))
        mu, ez2 = z.sum((0, 1)) / M, (z * z).sum((0, 1)) / M
        var = ez2 - mu * mu
        dmu = rnd(mu)
        dvar = rnd(ez2) + 2 * mu.abs() * dmu + rnd(mu * mu, dmu)
        dvar = dvar + rnd(var, dvar)
    is_ = (var + EPS).rsqrt()
    ris = 0.5 * dvar / (var + EPS) + 3 * u_
    sc = gamma * is_
    dsc = sc.abs() * (ris + u_)
    sh = beta - mu * sc
    dsh = u_ * sh.abs() + mu.abs() * dsc + sc.abs() * dmu + u_ * (mu * sc).abs()
    # ---- forward tables
    S = z.sum(1)
    Sm = S / HW
    m = sc * Sm + sh
    dm_ = Sm.abs() * (dsc + 2 * u_ * sc.abs()) + dsh + u_ * m.abs()
    mb = _rb(m)
    t1 = mb @ W1.T + b1
    dt1 = (dm_ + b_ * m.abs()) @ W1.abs().T + (C + 3) * u_ * (mb.abs() @ W1.abs().T + b1.abs())
    assert not bool((t1.abs() <= dt1).any()), "an fc1 output is undecidable: choose other inputs"
    h = t1.clamp_min(0)
    hb = _rb(h)
    t2 = hb @ W2.T + b2
    Cr = W1.shape[0]
    dt2_ = (dt1 + b_ * h) @ W2.abs().T + (Cr + 3) * u_ * (hb @ W2.abs().T + b2.abs())
    s = torch.sigmoid(t2)
    q = s * (1 - s)
    ds_ = q * dt2_ + 6 * u_ * s
    # ---- y and the mask
    sn = s[:, None, :]
    uu = sc * z + sh
    du_ = z.abs() * dsc + dsh + u_ * uu.abs()
    v = uu * sn + res
    dv = sn * du_ + uu.abs() * ds_[:, None, :] + u_ * v.abs()
    ex = v.abs() <= dv
    y = v.clamp_min(0)
    out = dict(S=S, s=s, s_b=ds_, h=h, h_b=dt1, y=y, y_b=b_ * y + (1 + b_) * dv, ex=ex,
               mask=v > 0)
    if running:
        return out
    # ---- backward tables
    g = dy * (v > 0)
    mv = dy.abs() * ex
    G1, G2 = g.sum(1), (g * z).sum(1)
    G1b, G2b = mv.sum(1), (mv * z.abs()).sum(1)
    dsg = sc * G2 + sh * G1
    ddsg = (G2.abs() * dsc + G1.abs() * dsh + sc.abs() * G2b + sh.abs() * G1b
            + u_ * ((sh * G1).abs() + dsg.abs()))
    dt2 = dsg * q
    ddt2 = q * ddsg + dsg.abs() * (ds_ + 2 * u_ * q) + u_ * dt2.abs()
    dtb = _rb(dt2)
    hpos = (h > 0).double()
    dh = (dtb @ W2) * hpos
    ddh = ((ddt2 + b_ * dt2.abs()) @ W2.abs() + (C + 3) * u_ * (dtb.abs() @ W2.abs())) * hpos
    dhb = _rb(dh)
    dm = dhb @ W1
    ddm = (ddh + b_ * dh.abs()) @ W1.abs() + (Cr + 3) * u_ * (dhb.abs() @ W1.abs())
    i0 = t["init"].double()
    r = (N + 2) * u_
    out.update(
        G=torch.stack([G1, G2]), G_b=torch.stack([G1b, G2b]),
        dw2=i0 + dt2.T @ h, dw2_b=ddt2.T @ h + dt2.abs().T @ dt1 + r * (dt2.abs().T @ h + i0.abs()),
        dw1=i0 + dh.T @ m, dw1_b=ddh.T @ m.abs() + dh.abs().T @ dm_
        + r * (dh.abs().T @ m.abs() + i0.abs()),
        db2=i0 + dt2.sum(0), db2_b=ddt2.sum(0) + r * (dt2.abs().sum(0) + i0.abs()),
        db1=i0 + dh.sum(0), db1_b=ddh.sum(0) + r * (dh.abs().sum(0) + i0.abs()))
    # ---- the BatchNorm sums, dgamma, dbeta, dz
    e1, e2 = s * G1 + dm, s * G2 + dm * Sm
    T1, T2 = e1.sum(0), e2.sum(0)
    a1, a2 = (s * G1).abs() + dm.abs(), (s * G2).abs() + (dm * Sm).abs()
    dT1 = (G1.abs() * ds_ + ddm + s * G1b + u_ * a1).sum(0) + (N + 1) * u_ * a1.sum(0)
    dT2 = ((G2.abs() * ds_ + Sm.abs() * ddm + s * G2b + 4 * u_ * a2).sum(0)
           + (N + 1) * u_ * a2.sum(0))
    inner = T2 - mu * T1
    dinner = dT2 + mu.abs() * dT1 + T1.abs() * dmu + u_ * (inner.abs() + (mu * T1).abs())
    sxh = is_ * inner
    dsxh = is_ * dinner + sxh.abs() * (ris + u_)
    k1, k2 = T1 / M, sxh / M
    dk1, dk2 = dT1 / M + 2 * u_ * k1.abs(), dsxh / M + 2 * u_ * k2.abs()
    dmh = dm[:, None, :] / HW
    du = g * sn + dmh
    ddu = (g.abs() * ds_[:, None, :] + ddm[:, None, :] / HW + 2 * u_ * dmh.abs() + u_ * du.abs())
    xh = (z - mu) * is_
    dxh = is_ * (dmu + u_ * (z - mu).abs()) + xh.abs() * (ris + u_)
    inn = du - k1 - xh * k2
    dinn = (ddu + dk1 + u_ * (du - k1).abs() + k2.abs() * dxh + xh.abs() * dk2
            + u_ * (inn.abs() + (xh * k2).abs()))
    dz = sc * inn
    ddz = sc.abs() * dinn + inn.abs() * dsc + u_ * dz.abs()
    out.update(dbeta=i0 + T1, dbeta_b=dT1 + 2 * u_ * (T1.abs() + i0.abs()),
               dgamma=i0 + sxh, dgamma_b=dsxh + 2 * u_ * (sxh.abs() + i0.abs()),
               dz=dz, dz_b=b_ * dz.abs() + (1 + b_) * ddz, dres=g)
    return out


def _inputs(N, P, Q, C, Cr, seed):
    HW = P * Q
    g = torch.Generator().manual_seed(seed)
    t = dict(z=int_tensor((N, HW, C), -4, 4, seed).double(),
             res=int_tensor((N, HW, C), -4, 4, seed + 1).double(),
             dy=int_tensor((N, HW, C), -3, 3, seed + 2).double(),
             w1=gauss_bf16((Cr, C), seed + 3, C ** -0.5),
             # (fc1 biases of both signs away from 0: which h are positive is then decidable)
             b1=gauss_bf16((Cr,), seed + 4, 0.25) + 1.5 * (1 - 2 * (torch.arange(Cr) % 2)),
             w2=gauss_bf16((C, Cr), seed + 5, Cr ** -0.5), b2=gauss_bf16((C,), seed + 6, 0.5),
             gamma=(torch.rand(C, generator=g) + 0.5)
             * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float(),
             beta=torch.randn(C, generator=g) * 0.1,
             rm=torch.randn(C, generator=g) * 0.3, rv=torch.rand(C, generator=g) * 4 + 2,
             init=torch.tensor(3.0))
    return t


GRADS = ("dw1", "db1", "dw2", "db2", "dgamma", "dbeta")


def _alloc(N, HW, C, Cr, init):
    """NaN-filled outputs (mask: 0xAA) and gradient slices pre-filled with ``init``."""
    nan = lambda *s, dt=torch.float32: torch.full(s, float("nan"), device=DEV, dtype=dt)
    o = dict(coef=nan(6, C), S=nan(N, C), s=nan(N, C), h=nan(N, Cr), y=nan(N, HW, C, dt=BF16),
             mask=torch.full((N, HW, C // 8), 0xAA, device=DEV, dtype=torch.uint8),
             G=nan(2, N, C), dt2=nan(N, C), dh=nan(N, Cr), dm=nan(N, C),
             dz=nan(N, HW, C, dt=BF16), dres=nan(N, HW, C, dt=BF16))
    for k, s in zip(GRADS, ((Cr, C), (Cr,), (C, Cr), (C,), (C,), (C,))):
        o[k] = torch.full(s, init, device=DEV)
    return o


def _launch(nat, shape, t, o, running, bwd, red=None):
    from ddp_amd.ops.common import ptr, stream_handle, workspace, stat_replicas
    N, P, Q, C, Cr = shape
    red = C // Cr if red is None else red
    dv = lambda x, dt=torch.float32: x.to(dt).to(DEV).contiguous()
    z, res, dy = (dv(t[k], BF16) for k in ("z", "res", "dy"))
    stats = torch.zeros(stat_replicas(), 2, C, device=DEV)
    stats[0, 0], stats[0, 1] = dv(t["z"].sum((0, 1))), dv((t["z"] ** 2).sum((0, 1)))
    p = {k: dv(t[k]) for k in ("w1", "b1", "w2", "b2", "gamma", "beta", "rm", "rv")}
    ws, st = workspace(torch.device(DEV)), stream_handle()
    if not bwd:
        nat.se_fwd(N, P, Q, C, red, EPS, ptr(z), ptr(res), ptr(stats), ptr(p["gamma"]),
                   ptr(p["beta"]), ptr(o["coef"]), ptr(p["w1"]), ptr(p["b1"]), ptr(p["w2"]),
                   ptr(p["b2"]), ptr(o["S"]), ptr(o["s"]), ptr(o["h"]), ptr(o["y"]),
                   ptr(o["mask"]), ptr(ws), ws.numel(), st, running_mean=ptr(p["rm"]),
                   running_var=ptr(p["rv"]), momentum=0.0, use_running=int(running))
    else:
        nat.se_bwd(N, P, Q, C, red, ptr(z), ptr(dy), ptr(o["mask"]), ptr(o["coef"]), ptr(p["w1"]),
                   ptr(p["w2"]), ptr(o["S"]), ptr(o["s"]), ptr(o["h"]), ptr(o["G"]), ptr(o["dt2"]),
                   ptr(o["dh"]), ptr(o["dm"]), ptr(o["dw1"]), ptr(o["db1"]), ptr(o["dw2"]),
                   ptr(o["db2"]), ptr(o["dgamma"]), ptr(o["dbeta"]), ptr(o["dz"]), ptr(o["dres"]),
                   ptr(ws), ws.numel(), st)
    torch.cuda.synchronize()


def _bits(mask, C):
    m = mask.cpu().to(torch.int32).unsqueeze(-1) >> torch.arange(8, dtype=torch.int32) & 1
    return m.reshape(*mask.shape[:-1], C).bool()


@pytest.mark.parametrize("N,P,Q,C,Cr,running",
                         [c + (False,) for c in CASES] + [CASES[2] + (True,)])
def test_se_per_element(native_ext, N, P, Q, C, Cr, running):
    # (C = 64: the seed whose reference has no undecidable element among its 64)
    t = _inputs(N, P, Q, C, Cr, 900 + C + N + 100 * (C == 64))
    r = se_reference(t, running)
    o = _alloc(N, P * Q, C, Cr, float(t["init"]))
    for bwd in (False,) if running else (False, True):
        _launch(native_ext, (N, P, Q, C, Cr), t, o, running, bwd)
    assert_within(o["S"], r["S"], 0.0, what="S")
    assert bool(((_bits(o["mask"], C) == r["mask"]) | r["ex"]).all()), "mask bits"
    for k in ("h", "s", "y") + (() if running else ("G", "dz") + GRADS):
        ex = r["ex"] if k in ("y", "dz") else None
        print(k, assert_within(o[k], r[k], r[k + "_b"], exclude=ex, what=k))
    if not running:
        assert_within(o["dres"], r["dres"], 0.0, exclude=r["ex"], what="dres")


@pytest.mark.parametrize("C,red", [(32, 2), (96, 2), (4096, 32), (256, 32), (2048, 8), (64, 3)])
def test_se_refusals(native_ext, C, red):
    """C below, off and above the range; Cr = 8 and 256; a reduction that does not divide C:
    se_ok is False, both launchers raise ValueError and every output keeps its fill."""
    from ddp_amd.ops.layers import SESpec
    assert native_ext.se_ok(2, 2, 2, 192, 4) and not native_ext.se_ok(2, 2, 2, C, red)
    Cr = C // red
    t = _inputs(2, 2, 2, C, Cr, 5)
    o = _alloc(2, 4, C, Cr, 3.0)
    for bwd in (False, True):
        with pytest.raises(ValueError, match="invalid arguments"):
            _launch(native_ext, (2, 2, 2, C, Cr), t, o, False, bwd, red)
    torch.cuda.synchronize()
    for k, v in o.items():
        keep = v == 0xAA if k == "mask" else (v == 3.0 if k in GRADS else torch.isnan(v.float()))
        assert bool(keep.all()), k
    with pytest.raises(ValueError, match="Squeeze-and-Excitation is served"):
        SESpec(torch.nn.Linear(C, Cr), torch.nn.Linear(Cr, C), red)


@pytest.mark.parametrize("groups,project", [(1, False), (32, True)])
def test_se_bottleneck_matches_cpu(native_ext, groups, project):
    """An identity and a projection SE Bottleneck (C = 256) at 8 x 8 x 8 against the same module's
    CPU fp32 forward and backward: loss within 5 %, cosine > 0.97 on the input gradient and on
    every parameter gradient (tests/test_gpu_resnext.py's criteria)."""
    from ddp_amd.models.resnet import Bottleneck
    from ddp_amd.optim import FusedSGD
    from ddp_amd.ops.layers import global_avg_pool
    torch.manual_seed(0)
    cin, ds = (128 if project else 256), None
    if project:
        ds = torch.nn.Sequential(torch.nn.Conv2d(128, 256, 1, bias=False), torch.nn.BatchNorm2d(256))
    cpu = Bottleneck(cin, 64, downsample=ds, groups=groups, base_width=4 if groups > 1 else 64,
                     se_reduction=16)
    gpu = copy.deepcopy(cpu).cuda()
    FusedSGD(gpu.parameters(), lr=0.1).zero_grad()
    x = torch.randn(8, cin, 8, 8).to(BF16).float().requires_grad_(True)
    w = torch.randn(8, 256)
    out_c = (cpu(x).mean((2, 3)) * w).sum()
    out_c.backward()
    xn = x.detach().permute(0, 2, 3, 1).contiguous().to(BF16).cuda().requires_grad_(True)
    out_g = (global_avg_pool(gpu.forward_fused(xn)).float() * w.cuda()).sum()
    out_g.backward()
    torch.cuda.synchronize()
    assert abs(float(out_g.detach()) - float(out_c.detach())) < 0.05 * max(1.0, abs(float(out_c.detach())))
    pairs = [("input", xn.grad.float().cpu(), x.grad.permute(0, 2, 3, 1))]
    pairs += [(n, pg.grad.cpu(), pc.grad) for (n, pc), pg in zip(cpu.named_parameters(),
                                                                gpu.parameters())]
    cos = {n: float(torch.dot(a.reshape(-1), b.reshape(-1)) / (a.norm() * b.norm() + 1e-20))
           for n, a, b in pairs}
    assert len(cos) == (17 if project else 14) and min(cos.values()) > 0.97, cos


def test_small_se_resnet_graph_replay_matches_eager_steps(native_ext):
    """ResNet((1, 1, 1, 1), se_reduction=16) on 32 x 32 (layer4 is 1 x 1), batch 8, with the
    default 1000-way head as the mains run it (the GEMM head takes multiples of 8 classes): three
    replays of the captured step give the losses and the weights of three eager steps from the
    same state (2 % on a loss as tests/test_gpu_mobilenet.py; weights to 1e-3 of their scale:
    the statistics atomics reorder fp32 sums between runs)."""
    from ddp_amd.models.resnet import ResNet
    from ddp_amd.engine import CrossEntropyLoss, TrainStep
    from ddp_amd.optim import FusedSGD
    from ddp_amd.data import SyntheticCIFAR10, DeviceLoader
    torch.manual_seed(5)
    model = ResNet((1, 1, 1, 1), se_reduction=16).cuda()
    opt = FusedSGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    ld = DeviceLoader(SyntheticCIFAR10(True, n=64), 8, "cuda")
    st = TrainStep(model, opt, CrossEntropyLoss(), ld, use_graph=True)
    st.warmup(2)
    st.capture()
    st.pop_loss()
    bufs = [b for b in model.buffers()]
    snap = (opt.arena.data.clone(), opt.momentum_buffer.clone(), ld.cursor.clone(),
            [b.clone() for b in bufs])
    eager = []
    for _ in range(3):
        st._body()
        eager.append(st.pop_loss())
    w_eager = opt.arena.data.clone()
    opt.arena.data.copy_(snap[0]); opt.momentum_buffer.copy_(snap[1]); ld.cursor.copy_(snap[2])
    for b, v in zip(bufs, snap[3]):
        b.copy_(v)
    for sp in model.fused_plan():
        sp._packed_version = None
        sp.maybe_pack()
    for i in range(3):
        st.step()
        v = st.pop_loss()
        assert v == v and abs(v - eager[i]) < 2e-2 * max(1.0, abs(eager[i])), (i, v, eager)
    assert len(set(eager)) == 3
    err = float((opt.arena.data - w_eager).abs().max())
    assert err < 1e-3 * float(w_eager.abs().max()), err
