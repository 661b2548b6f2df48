"""Per-element tests of the VGG input block's kernels (conv_l0.hip) in their lane layout: a lane
owns one pool window x four channels, the conv is issued as mfma(pixels, channels), the pool, the
code and the winner's z are taken over four registers, and the fused backward feeds its dz
registers to the weight-gradient MFMA. A wrong pixel order, channel permutation, code byte or
patch offset moves whole elements, so everything discrete is demanded exactly and everything
else per element.

Operands are integer valued: x and w in {-1, 0, 1}, bias in {-3..3}. z is then an exact integer
with |z| <= 30 (27 products + bias), a bf16 number, and equal z give equal y, so ties for a
window's maximum are decided exactly (gamma > 0: the first maximum of z is the first maximum of
y). The reference (fp64, CPU) decides every window: ``_ref`` asserts that no pooled value lies
within 16 * 2**-24 * (|z * scale| + |shift| + 1) of zero, so no element is excluded anywhere.

Shapes (N, H, W), the smallest at which each part can go wrong:
  (1, 2, 8)     one tile, every pixel on a border; the pixel ordering of both MFMA operands
                decides every dW element
  (2, 4, 8)     4 tiles, one block
  (3, 32, 32)   odd N, 192 tiles, a partial last block
  (72, 32, 32)  4608 tiles on 4096 waves: some waves own two tiles; 1024 blocks
"""
import pytest
import torch
import torch.nn.functional as F

from exactness import BF16_EPS as b_, FP32_EPS as u_, assert_exact, assert_within, dot_bound, \
    int_tensor, mismatches
from test_gpu_elementwise import EPS, bn_fwd_terms, bn_out_bound

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
NHWC = ("n", "h", "w", "c")
K = 64
SHAPES = [(1, 2, 8), (2, 4, 8), (3, 32, 32), (72, 32, 32)]
_REF, _FWD, _BWD = {}, {}, {}


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _cv(v):
    return v.view(1, -1, 1, 1)


def _win(v):
    """NCHW -> [N][C][H/2][W/2][4], window positions in bn_act.hip's order d = 2r + c."""
    N, C, H, W = v.shape
    return v.reshape(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(
        N, C, H // 2, W // 2, 4)


def _unwin(v):
    """Inverse of ``_win``."""
    N, C, Ho, Wo, _ = v.shape
    return v.reshape(N, C, Ho, Wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, 2 * Ho, 2 * Wo)


def _ref(shape, bias):
    """fp64 reference of the block on the integer operands (CPU), computed once per case and
    left unchanged: z, its sums, the BatchNorm terms, the pooled output with its bound, the first
    maximum of every window and the code it implies."""
    key = (shape, bias)
    if key in _REF:
        return _REF[key]
    N, H, W = shape
    x = int_tensor((N, 3, H, W), -1, 1, 7)
    w = int_tensor((K, 3, 3, 3), -1, 1, 8)
    b = int_tensor((K,), -3, 3, 9) if bias else None
    g = torch.Generator().manual_seed(12)
    gamma = torch.rand(K, generator=g) + 0.5
    beta = torch.randn(K, generator=g) * 0.1
    bd = b.double() if bias else None
    z = F.conv2d(x.double(), w.double(), bd, 1, 1)
    za = F.conv2d(x.abs().double(), w.abs().double(), bd.abs() if bias else None, 1, 1)
    assert float(z.abs().max()) <= 30 and bool((z == z.round()).all())
    t = bn_fwd_terms(z, gamma, beta)
    t["z"] = z
    zw, yw = _win(z), _win(t["y"])
    top = zw.max(-1, keepdim=True).values
    eq = zw == top
    first = eq & (eq.int().cumsum(-1) == 1)
    pos = (first.int() * torch.arange(4)).sum(-1)          # first maximum of z in window order
    ymax = yw.max(-1).values                                # the pooled value before ReLU
    # the reference decides every window: no pooled value within 16 fp32 roundings of zero
    margin = 16 * u_ * ((top.squeeze(-1) * _cv(t["sc"])).abs() + _cv(t["sh"].abs()) + 1)
    assert bool((ymax.abs() > margin).all()), "a pooled value too close to zero: other inputs"
    assert bool((ymax == yw.gather(-1, pos.unsqueeze(-1)).squeeze(-1)).all())  # (gamma > 0)
    code = torch.where(ymax > 0, pos, torch.full_like(pos, 4))
    out, out_bound = bn_out_bound(t, True, True)
    zb = z.reshape(N, K, -1)
    r = dict(x=x, w=w, b=b, gamma=gamma, beta=beta, z=z, t=t, code=code, pos=pos,
             zsel=zw.gather(-1, pos.unsqueeze(-1)).squeeze(-1), out=out, out_bound=out_bound,
             s1=zb.sum((0, 2)), a1=za.reshape(N, K, -1).sum((0, 2)), s2=(zb * zb).sum((0, 2)),
             ties=float((eq.sum(-1) > 1).double().mean()), cut=float((code == 4).double().mean()))
    _REF[key] = r
    return r


def _operands(r, shape):
    from ddp_amd.ops.layers import ConvBNActSpec
    N, H, W = shape
    conv = torch.nn.Conv2d(3, K, 3, 1, 1, bias=True).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(r["w"])
        conv.bias.copy_(r["b"] if r["b"] is not None else torch.zeros(K))
    spec = ConvBNActSpec(conv, None, cin_pad=8)
    spec.maybe_pack()
    xn = torch.zeros(N, H, W, 8, dtype=BF16)
    xn[..., :3] = _nhwc(r["x"]).to(BF16)
    return conv, spec, xn.to(DEV)


def _forward(nat, shape, bias, xn=None):
    """One l0_fwd call on the case's operands (``xn``: another input); outputs pre-filled."""
    from ddp_amd.ops.common import ptr, stream_handle
    N, H, W = shape
    r = _ref(shape, bias)
    conv, spec, x0 = _operands(r, shape)
    xn = x0 if xn is None else xn
    g = spec.geom(N, H, W)
    assert nat.l0_ok(g)
    shp = (N, H // 2, W // 2, K)
    f = dict(conv=conv, spec=spec, xn=xn, g=g, bias=conv.bias if bias else None,
             gamma=r["gamma"].to(DEV), beta=r["beta"].to(DEV),
             stats=torch.zeros(16 * 2 * K, device=DEV),
             coef=torch.full((6 * K,), float("nan"), device=DEV),
             y=torch.full(shp, float("nan"), device=DEV, dtype=BF16),
             code=torch.full(shp, 0xEE, device=DEV, dtype=torch.uint8),
             zw=torch.full(shp, float("nan"), device=DEV, dtype=BF16))
    nat.l0_fwd(g, ptr(xn), ptr(spec.wc), ptr(f["bias"]), EPS, 1, ptr(f["stats"]), ptr(f["gamma"]),
               ptr(f["beta"]), ptr(f["coef"]), ptr(f["y"]), ptr(f["code"]), ptr(f["zw"]),
               stream_handle())
    torch.cuda.synchronize()
    return f


def _fwd(nat, shape, bias):
    key = (shape, bias)
    if key not in _FWD:
        _FWD[key] = _forward(nat, shape, bias)
    return _FWD[key]


def _decode(code, shape):
    """The code bytes [window][g'][j'][v'] -> [N][C = j'*16 + 4g' + v'][H/2][W/2]."""
    N, H, W = shape
    c = code.cpu().view(N, H // 2, W // 2, 4, 4, 4).permute(0, 1, 2, 4, 3, 5).reshape(
        N, H // 2, W // 2, K)
    return c.permute(0, 3, 1, 2).long()


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_statistics_exact(native_ext, shape, bias):
    """sum z and sum z^2 of the statistics pass: integers, exact in any order."""
    r, f = _ref(shape, bias), _fwd(native_ext, shape, bias)
    st = f["stats"].view(16, 2 * K).sum(0).cpu()
    assert_exact(st[:K], r["s1"], r["a1"], ("k",), "sum z")
    assert_exact(st[K:], r["s2"], r["s2"], ("k",), "sum z^2")


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_discrete_outputs(native_ext, shape):
    """Every window and channel: code = the first maximum of z in window order where the
    reference's pooled y > 0, 4 elsewhere; y exactly 0 where the code is 4; zw = z of the coded
    pixel bit for bit wherever code < 4."""
    r, f = _ref(shape, True), _fwd(native_ext, shape, True)
    print(f"l0 layout {shape}: ties {r['ties']:.3f} cut {r['cut']:.3f}")
    assert r["ties"] > 0.05 and r["cut"] > 0.01  # the inputs exercise both rules
    code = _decode(f["code"], shape)
    bad = code != r["code"]
    assert not bool(bad.any()), (int(bad.sum()), torch.nonzero(bad)[:8].tolist(),
                                 code[bad][:8].tolist(), r["code"][bad][:8].tolist())
    y = f["y"].cpu().permute(0, 3, 1, 2)
    zero = torch.zeros_like(y)
    assert not bool(mismatches(y[code == 4], zero[code == 4]).any()), "y where the code is 4"
    ok = code < 4
    zw = f["zw"].cpu().permute(0, 3, 1, 2)
    want = r["zsel"].to(BF16)
    assert float((want.double() - r["zsel"]).abs().max()) == 0.0  # z is a bf16 number
    assert not bool(mismatches(zw[ok], want[ok]).any()), "zw at the coded pixel"


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_y_per_element(native_ext, shape):
    """Every pooled y within its bound. The kernel's expressions are bn_act.hip's (l0_fwd_kernel
    setup = finalize: mu = S1 / M, var = max(S2 / M - mu * mu, 0), is = rsqrtf(var + eps),
    sc = gamma * is, sh = beta - mu * sc; epilogue y = z * sc + sh, ReLU, max, one bf16 store),
    so the count is the table of test_gpu_elementwise.bn_fwd_terms: 2 roundings on mu, 8 on var,
    rsqrt 1 ulp, 1 on sc, 2 on sh, 2 on y (z itself is exact here), then 2**-8 |ref| for the
    store (bn_out_bound; ReLU and max are 1-Lipschitz). The statistics the kernel folds are the
    exact integer sums (test_statistics_exact), for which the table allows one rounding each."""
    r, f = _ref(shape, True), _fwd(native_ext, shape, True)
    worst = assert_within(f["y"], _nhwc(r["out"]), _nhwc(r["out_bound"]), NHWC, what="y")
    print(f"l0 layout {shape}: y worst |err|/bound {worst:.3f}")


def test_nan_input_marks_every_window(native_ext):
    """One NaN input pixel makes the statistics of every channel NaN (0 * NaN = NaN in the
    conv): every code byte 0xFF, every y NaN."""
    shape = (2, 4, 8)
    r = _ref(shape, True)
    _, _, xn = _operands(r, shape)
    xn[0, 1, 2, 1] = float("nan")
    f = _forward(native_ext, shape, True, xn)
    assert bool(torch.isnan(f["stats"].view(16, 2 * K).sum(0)).all())
    assert bool((f["code"] == 0xFF).all()), f["code"].unique().tolist()
    assert bool(torch.isnan(f["y"].float()).all())


def dz_terms(r, dyb):
    """fp64 dz = sc * (dyb - k1 - xhat * k2) for the routed gradient ``dyb`` (NCHW) and the bound
    of the kernels' evaluation (conv_l0.hip l0_sums_kernel, l0_bwd_body), with u = 2**-24, the
    forward's terms (rsc, ris, dmu, dxh: test_gpu_elementwise.bn_fwd_terms) and

    | quantity                                  | roundings                                   |
    |-------------------------------------------|---------------------------------------------|
    | S1 = sum dyb (M terms, any order)         | M                                           |
    | S2 = sum dyb * ((zw - mu) * is)           | dxh on xhat, M + 1 (product, any order)     |
    | k = S * inv_m, inv_m = 1 / M              | 2                                           |
    | cz = -sc * k2 * is                        | rsc, dk2, ris, 2 products                   |
    | P = k2 * is * mu                          | dk2, ris, dmu, 2 products                   |
    | c0 = sc * (P - k1)                        | dP, dk1, 1 subtraction; rsc, 1 product      |
    | dz = sc * dyb + (z * cz + c0)             | rsc + 1 product; 1 product; 2 additions     |
    | store                                     | one bf16 rounding                           |

    z and dyb are exact. A fused multiply-add only removes roundings."""
    t, z = r["t"], r["z"]
    M = t["M"]
    sm = lambda v: v.sum((0, 2, 3))
    xh, dxh = t["xh"], t["dxh"]
    sc, is_, mu, rsc, ris = t["sc"], t["is_"], t["mu"], t["rsc"], t["ris"]
    dmu = 2 * u_ * mu.abs()
    S1, S2 = sm(dyb), sm(dyb * xh)
    dS1 = M * u_ * sm(dyb.abs())
    dS2 = sm(dyb.abs() * dxh) + (M + 1) * u_ * sm((dyb * xh).abs())
    k1, k2 = S1 / M, S2 / M
    dk1, dk2 = dS1 / M + 2 * u_ * k1.abs(), dS2 / M + 2 * u_ * k2.abs()
    cz = -sc * k2 * is_
    dcz = cz.abs() * (rsc + ris + 2 * u_) + (sc * is_).abs() * dk2
    P = k2 * is_ * mu
    dP = (is_ * mu).abs() * dk2 + P.abs() * (ris + 2 * u_) + (k2 * is_).abs() * dmu
    c0 = sc * (P - k1)
    dc0 = sc.abs() * (dP + dk1 + u_ * (P - k1).abs()) + c0.abs() * (rsc + u_)
    A, B = _cv(sc) * dyb, z * _cv(cz)
    dz = A + B + _cv(c0)
    ddz = (A.abs() * _cv(rsc + u_) + z.abs() * _cv(dcz) + u_ * B.abs() + _cv(dc0)
           + u_ * (B + _cv(c0)).abs() + u_ * dz.abs())
    ref = _cv(sc) * (dyb - _cv(k1) - xh * _cv(k2))
    assert float((ref - dz).abs().max()) <= 1e-9 * max(1.0, float(ref.abs().max()))
    return ref, b_ * ref.abs() + (1 + b_) * ddz


def _backward(nat, shape):
    """The stored-dz backward of the case (bias on): dy in {-2..2}, outputs pre-filled with NaN."""
    if shape in _BWD:
        return _BWD[shape]
    from ddp_amd.ops.common import ptr, stream_handle
    N, H, W = shape
    f = _fwd(nat, shape, True)
    dy = int_tensor((N, K, H // 2, W // 2), -2, 2, 10)
    dyn = _nhwc(dy).to(BF16).to(DEV)
    sums = torch.zeros(16 * 2 * K, device=DEV)
    dz = torch.full((N, H, W, K), float("nan"), device=DEV, dtype=BF16)
    dg, db = torch.zeros(K, device=DEV), torch.zeros(K, device=DEV)
    coef = f["coef"].clone()
    rc = nat.l0_bwd(f["g"], ptr(f["xn"]), ptr(f["spec"].wc), ptr(f["bias"]), EPS, 1, ptr(coef),
                    ptr(dyn), ptr(sums), ptr(dz), ptr(dg), ptr(db), ptr(f["code"]), ptr(f["zw"]),
                    stream_handle())
    torch.cuda.synchronize()
    assert rc == 0
    _BWD[shape] = dict(dy=dy, dyn=dyn, sums=sums, dz=dz, coef=coef)
    return _BWD[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_stored_dz_per_element(native_ext, shape):
    """Every dz element of l0_bwd_kernel<1> within the bound of ``dz_terms``, against fp64 built
    from the reference's own routing (the pooled gradient goes to the reference's first maximum
    where its pooled y > 0); an unwritten element stays NaN and fails."""
    r = _ref(shape, True)
    bw = _backward(native_ext, shape)
    take = F.one_hot(r["code"], 5)[..., :4].double()         # [N][C][Ho][Wo][4]
    dyb = _unwin(take * bw["dy"].double().unsqueeze(-1))
    ref, bound = dz_terms(r, dyb)
    worst = assert_within(bw["dz"], _nhwc(ref), _nhwc(bound), NHWC, what="dz")
    print(f"l0 layout {shape}: dz worst |err|/bound {worst:.3f}")


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_backward_fused_dw_per_element(native_ext, shape):
    """Every dW element of the fused form (dz chained from registers into the weight-gradient
    MFMA) within dot_bound(n = N * H * W, no bf16 rounding) of the fp64 contraction of the stored
    dz with x, for both weight layouts. Both calls fold the same BN-backward sums."""
    from ddp_amd.ops.common import ptr, stream_handle, weight_krsc, workspace
    nat = native_ext
    N, H, W = shape
    r, f = _ref(shape, True), _fwd(nat, shape, True)
    bw = _backward(nat, shape)
    assert not bool(torch.isnan(bw["dz"].float()).any())
    d = bw["dz"].cpu().double().reshape(N, H * W, K)
    cols = F.unfold(r["x"].double(), 3, padding=1)            # [N][27 = (c, r, s)][H * W]
    ref = torch.einsum("npk,ncp->kc", d, cols).reshape(K, 3, 3, 3)
    absref = torch.einsum("npk,ncp->kc", d.abs(), cols.abs()).reshape(K, 3, 3, 3)
    bound = dot_bound(ref, absref, N * H * W, bf16_roundings=0)
    ws = workspace(f["xn"].device)
    for layout in (torch.channels_last, torch.contiguous_format):  # [K][R][S][3] and [K][3][R][S]
        dw = torch.zeros_like(f["conv"].weight, memory_format=layout)
        coef = f["coef"].clone()
        dg, db = torch.zeros(K, device=DEV), torch.zeros(K, device=DEV)
        g = f["spec"].geom(N, H, W, weight_krsc(dw))
        rc = nat.l0_bwd(g, ptr(f["xn"]), ptr(f["spec"].wc), ptr(f["bias"]), EPS, 1, ptr(coef),
                        ptr(bw["dyn"]), ptr(bw["sums"]), 0, ptr(dg), ptr(db), ptr(f["code"]),
                        ptr(f["zw"]), stream_handle(), sums_ready=1, dw=ptr(dw), ws=ptr(ws),
                        ws_elems=ws.numel())
        torch.cuda.synchronize()
        assert rc == 0
        worst = assert_within(dw.detach(), ref, bound, ("k", "c", "r", "s"), what=f"dW {layout}")
        print(f"l0 layout {shape} {layout}: dW worst |err|/bound {worst:.3f}")
        assert torch.equal(coef, bw["coef"])
