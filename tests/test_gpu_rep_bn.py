"""RepVGG block kernels (rep_bn.hip) against fp64, element for element (tests/exactness.py
assert_within): y, the coefficient tables, the running statistics, the emitted statistics of y,
dz3 / dz1 / dxid, dgamma / dbeta, k1 / k2; eval mode; the refusals.

The statistics tables are computed in fp64 from the bf16 inputs and passed in as two equal
replicas (their fp32 sum is exact), so the reference starts from the kernel's own inputs. The
backward gets the reference forward's y (bf16) as its mask source and the reference's (scale, mean,
invstd) rounded to fp32 as its table, and the fp64 backward uses those same values: g is a
function of the backward's inputs alone and nothing is excluded.

Bounds, counted from rep_bn.hip (u = 2**-24 per fp32 rounding, b = 2**-8 per bf16 store, M rows):

| quantity                                        | roundings                               |
|-------------------------------------------------|-----------------------------------------|
| mu = s1 / M                                     | 1                                       |
| var = max(s2 / M - mu * mu, 0)                  | 2 on s2 / M, 4 on mu^2                  |
| is = rsqrtf(var + eps)                          | (dvar / (var + eps) + 1) / 2; v_rsq: 2  |
| sc = gamma * is;  sh = beta - mu * sc           | 1;  2 on mu sc + 1                      |
| shift = (sh3 + sh1) + sh0                       | 2                                       |
| pre = fma(z3, sc3, fma(z1, sc1, fma(x, sc0, .)))| one per fma, of the magnitudes' sum     |
| running = (1 - m) * old + m * new               | 4 of the magnitudes' sum                |
| sum y, sum y^2 (fp32, any order)                | M + 2                                   |
| S = sum g;  T = sum fma(g, z - mu, T)           | M + 2;  M + 3                           |
| s2 = is * T; k1 = S / M; k2 = s2 / M; w = is k2 | 1; 2; 2; 1                              |
| dz = sc * fma(-(z - mu), w, g - k1)             | sub, sub, fma, product; bf16 store      |
| dgamma += s2;  dbeta += S                       | 1                                       |
"""
import pytest
import torch

from exactness import BF16_EPS as b_, FP32_EPS as u_, assert_within, dot_bound, gauss_bf16

pytestmark = pytest.mark.gpu
f32v = lambda v: float(torch.tensor(v).double())  # the value the kernel gets as a float argument
DEV, BF16, EPS, MOM = "cuda", torch.bfloat16, f32v(1e-5), f32v(0.1)
SHAPES = [(1, 1, 1, 8), (2, 3, 5, 48), (4, 8, 8, 64), (2, 2, 2, 320), (16, 16, 16, 16)]
f32 = lambda t: t.float().double()  # rounded to fp32, as the kernel reads it


def _case(N, H, W, K, nbr, seed):
    """Inputs and the fp64 reference with its bounds, everything [M][K] / [K] fp64 on the CPU."""
    M, r = N * H * W, {}
    g = torch.Generator().manual_seed(seed)
    r["z"] = [gauss_bf16((M, K), seed + i, 1.5 - 0.4 * i, 0.3 * i - 0.2).double() for i in range(nbr)]
    r["gamma"] = [f32((torch.rand(K, generator=g) + 0.5) * (torch.randint(0, 2, (K,), generator=g) * 2 - 1))
                  for _ in range(nbr)]
    r["beta"] = [f32(torch.randn(K, generator=g) * 0.2) for _ in range(nbr)]
    r["run"] = [(f32(torch.randn(K, generator=g)), f32(torch.rand(K, generator=g) + 0.5)) for _ in range(nbr)]
    r["half"] = [torch.stack([z.sum(0), (z * z).sum(0)]).float() / 2 for z in r["z"]]
    r["dy"] = gauss_bf16((M, K), seed + 7).double()
    pre = pre_mag = torch.zeros(M, K, dtype=torch.float64)
    dpre = torch.zeros(M, K, dtype=torch.float64)
    r["coef"], r["coef_b"], r["new_run"], r["run_b"] = [], [], [], []
    for z, ga, be, half, (rm, rv) in zip(r["z"], r["gamma"], r["beta"], r["half"], r["run"]):
        s1, s2 = 2 * half[0].double(), 2 * half[1].double()
        mu = s1 / M
        var = (s2 / M - mu * mu).clamp_min(0)
        dmu, dvar = u_ * mu.abs(), 2 * u_ * s2 / M + 4 * u_ * mu * mu
        is_ = (var + EPS).rsqrt()
        ris = 0.5 * (dvar / (var + EPS) + u_) + 2 * u_
        sc = ga * is_
        sh = be - mu * sc
        rsc = ris + u_
        dsh = (mu * sc).abs() * (rsc + 2 * u_) + u_ * sh.abs()
        pre, pre_mag = pre + z * sc + sh, pre_mag + (z * sc).abs() + sh.abs()
        dpre = dpre + z.abs() * sc.abs() * rsc + dsh + 2 * u_ * sh.abs()
        r["coef"].append(torch.stack([sc, sh, mu, is_]))
        r["coef_b"].append(torch.stack([sc.abs() * rsc, dsh, dmu, ris * is_]))
        fac = M / (M - 1) if M > 1 else 1.0
        unb = var * fac
        r["new_run"].append(torch.stack([(1 - MOM) * rm + MOM * mu, (1 - MOM) * rv + MOM * unb]))
        r["run_b"].append(torch.stack([
            4 * u_ * ((1 - MOM) * rm.abs() + MOM * mu.abs()) + MOM * dmu,
            4 * u_ * ((1 - MOM) * rv + MOM * unb) + MOM * (dvar + 3 * u_ * var) * fac]))
    r["y"] = pre.clamp_min(0)
    r["ybf"] = r["y"].to(BF16)  # the backward's mask source
    r["y_b"] = b_ * r["y"] + (1 + b_) * (dpre + nbr * u_ * pre_mag)
    return r


def _backward_ref(r, M, tabs, init):
    """fp64 backward from the fp32 tables ``tabs`` [(sc, mu, is)] and the reference y as mask."""
    g = r["dy"] * (r["ybf"] > 0)
    S, dS = g.sum(0), (M + 2) * u_ * g.abs().sum(0)
    k1 = S / M
    dk1 = dS / M + 2 * u_ * k1.abs()
    out = []
    for z, (sc, mu, is_), (ig, ib) in zip(r["z"], tabs, init):
        d = z - mu
        T, dT = (g * d).sum(0), (M + 3) * u_ * (g * d).abs().sum(0)
        s2 = is_ * T
        ds2 = is_ * dT + u_ * s2.abs()
        k2 = s2 / M
        dk2 = ds2 / M + 2 * u_ * k2.abs()
        w = is_ * k2
        dw = is_ * dk2 + u_ * w.abs()
        inner = (g - k1) - d * w
        dinner = dk1 + u_ * (g - k1).abs() + d.abs() * (dw + u_ * w.abs()) + u_ * inner.abs()
        dz = sc * inner
        out.append(dict(dz=dz, dz_b=b_ * dz.abs() + (1 + b_) * (sc.abs() * dinner + u_ * dz.abs()),
                        k=torch.stack([k1, k2]), k_b=torch.stack([dk1, dk2]),
                        grads=torch.stack([ig + s2, ib + S]),
                        grads_b=torch.stack([ds2 + u_ * (ig + s2).abs(), dS + u_ * (ib + S).abs()])))
    return out


def _replicas(nat, half, K):
    t = torch.zeros(nat.stat_replicas(), 2, K)
    t[0] = t[1] = half
    return t.to(DEV)


@pytest.mark.parametrize("ostats", [False, True])
@pytest.mark.parametrize("nbr", [2, 3])
@pytest.mark.parametrize("N,H,W,K", SHAPES)
def test_rep_bn_per_element(native_ext, N, H, W, K, nbr, ostats):
    from ddp_amd.ops.common import ptr, stream_handle, workspace
    nat, M = native_ext, N * H * W
    r = _case(N, H, W, K, nbr, 900 + K + M)
    nan = lambda *s, dt=torch.float32: torch.full(s, float("nan"), device=DEV, dtype=dt)
    z = [t.to(DEV, BF16) for t in r["z"]]
    par = [(ga.float().to(DEV), be.float().to(DEV)) for ga, be in zip(r["gamma"], r["beta"])]
    run = [(a.float().to(DEV), v.float().to(DEV)) for a, v in r["run"]]
    stats = [_replicas(nat, h, K) for h in r["half"]]
    coef = [nan(6, K) for _ in range(nbr)]
    y, ost = nan(M, K, dt=BF16), torch.zeros(nat.stat_replicas(), 2, K, device=DEV)
    br = [(ptr(z[i]), ptr(stats[i]), ptr(par[i][0]), ptr(par[i][1]), ptr(run[i][0]), ptr(run[i][1]),
           MOM, EPS, ptr(coef[i]), 0, 0, 0) for i in range(nbr)]
    nat.rep_bn_fwd(N, H, W, K, br, ptr(y), ptr(ost) if ostats else 0, 0, stream_handle())
    torch.cuda.synchronize()
    print("y", assert_within(y, r["y"], r["y_b"], ("m", "k"), what="y"))
    for i in range(nbr):
        print(i, assert_within(coef[i][:4], r["coef"][i], r["coef_b"][i], what=f"coef table {i}"),
              assert_within(torch.stack(run[i]), r["new_run"][i], r["run_b"][i], what=f"running {i}"))
    if ostats:  # the sums of the kernel's own stored y
        yk = y.double().cpu()
        ref, mag = torch.stack([yk.sum(0), (yk * yk).sum(0)]), torch.stack([yk.sum(0), (yk * yk).sum(0)])
        print("ostats", assert_within(ost.double().sum(0), ref, dot_bound(ref, mag, M + 2, 0),
                                      what="statistics of y"))
    else:
        assert not bool(ost.any())

    # ---- backward: reference y as the mask source, the reference tables rounded to fp32
    tabs = [tuple(f32(r["coef"][i][j]) for j in (0, 2, 3)) for i in range(nbr)]
    gen = torch.Generator().manual_seed(5)
    init = [(f32(torch.randn(K, generator=gen)), f32(torch.randn(K, generator=gen))) for _ in range(nbr)]
    want = _backward_ref(r, M, tabs, init)
    for i, (sc, mu, is_) in enumerate(tabs):
        coef[i][0], coef[i][2], coef[i][3] = sc.to(DEV), mu.to(DEV), is_.to(DEV)
    grads = [torch.stack(g).float().to(DEV) for g in init]
    dz = [nan(M, K, dt=BF16) for _ in range(nbr)]
    ym, dy, ws = r["ybf"].to(DEV), r["dy"].to(DEV, BF16), workspace(torch.device(DEV))
    br = [b[:9] + (ptr(dz[i]), ptr(grads[i][0]), ptr(grads[i][1])) for i, b in enumerate(br)]
    nat.rep_bn_bwd(N, H, W, K, br, ptr(dy), ptr(ym), ptr(ws), ws.numel(), stream_handle())
    torch.cuda.synchronize()
    for i, wnt in enumerate(want):
        print(i, assert_within(dz[i], wnt["dz"], wnt["dz_b"], ("m", "k"), what=f"dz {i}"),
              assert_within(grads[i], wnt["grads"], wnt["grads_b"], what=f"dgamma / dbeta {i}"),
              assert_within(coef[i][4:], wnt["k"], wnt["k_b"], what=f"k1 / k2 {i}"))


def test_rep_bn_eval_uses_running_statistics(native_ext):
    from ddp_amd.ops.common import ptr, stream_handle
    N, H, W, K, nbr = 2, 3, 5, 48, 3
    r = _case(N, H, W, K, nbr, 77)
    z = [t.to(DEV, BF16) for t in r["z"]]
    dev = lambda ts: [t.float().to(DEV) for t in ts]
    ga, be, rm, rv = dev(r["gamma"]), dev(r["beta"]), dev(a for a, _ in r["run"]), dev(v for _, v in r["run"])
    coef = [torch.empty(6, K, device=DEV) for _ in range(nbr)]
    y = torch.full((N * H * W, K), float("nan"), device=DEV, dtype=BF16)
    br = [(ptr(z[i]), 0, ptr(ga[i]), ptr(be[i]), ptr(rm[i]), ptr(rv[i]), MOM, EPS, ptr(coef[i]), 0, 0, 0)
          for i in range(nbr)]
    native_ext.rep_bn_fwd(N, H, W, K, br, ptr(y), 0, 1, stream_handle())
    torch.cuda.synchronize()
    pre = mag = bound = 0
    for zi, g, bt, (m, v) in zip(r["z"], r["gamma"], r["beta"], r["run"]):
        sc = g * (v + EPS).rsqrt()
        sh = bt - m * sc
        pre, mag = pre + zi * sc + sh, mag + (zi * sc).abs() + sh.abs()
        bound = bound + (zi * sc).abs() * 4 * u_ + (m * sc).abs() * 6 * u_ + 3 * u_ * sh.abs()
    want = pre.clamp_min(0)
    print(assert_within(y, want, b_ * want + (1 + b_) * (bound + nbr * u_ * mag), what="eval y"))
    for i in range(nbr):
        assert torch.equal(rm[i].cpu().double(), r["run"][i][0]) and torch.equal(rv[i].cpu().double(), r["run"][i][1])


def test_rep_bn_refusals(native_ext):
    from ddp_amd.ops.common import ptr, stream_handle, workspace
    N, H, W, K = 2, 2, 2, 12
    assert not native_ext.rep_bn_ok(N, H, W, K) and native_ext.rep_bn_ok(N, H, W, 16)
    ones = torch.ones(64 * 2 * K + 6 * K, device=DEV)
    zb = torch.ones(N * H * W, K, device=DEV, dtype=BF16)
    outs = [torch.full((N * H * W, K), float("nan"), device=DEV, dtype=BF16) for _ in range(3)]
    br = [(ptr(zb), ptr(ones), ptr(ones), ptr(ones), 0, 0, 0.1, EPS, ptr(ones), ptr(outs[1 + i]),
           ptr(ones), ptr(ones)) for i in range(2)]
    ws = workspace(torch.device(DEV))
    with pytest.raises(RuntimeError, match="invalid arguments"):
        native_ext.rep_bn_fwd(N, H, W, K, br, ptr(outs[0]), 0, 0, stream_handle())
    with pytest.raises(RuntimeError, match="invalid arguments"):
        native_ext.rep_bn_bwd(N, H, W, K, br, ptr(zb), ptr(zb), ptr(ws), ws.numel(), stream_handle())
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o.float()).all()) for o in outs) and bool((ones == 1).all())
