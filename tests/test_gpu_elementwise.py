"""Bound-mode tests (tests/exactness.py assert_within) of the kernels whose arithmetic cannot be
made exact: BatchNorm forward / backward (bn_act.hip), softmax cross-entropy and the fused
classifier head (linear_ce.hip, conv_igemm.hip linear_head_bwd_kernel).

Every output element is compared with an fp64 reference of the same operation on the same
bf16-valued inputs. The bounds are first-order error bounds counted from the kernels' code, with
u = 2**-24 (one fp32 rounding, relative) and b = 2**-8 (one bf16 rounding); the tables beside the
bound functions name the lines. None of them was fitted to what the kernels return.

Transcendentals. Neither the HIP headers nor any document installed with ROCm states an ulp bound
for ``__expf`` / ``__logf`` / ``rsqrtf``. What the headers do state is their lowering
(__clang_hip_math.h): ``__expf(x) = __builtin_amdgcn_exp2f(0x1.715476p+0f * x)``, ``__logf =
__builtin_logf``, ``rsqrtf = __ocml_rsqrt_f32``, i.e. the v_exp_f32 / v_log_f32 / v_rsq_f32
instructions. The 1 ulp used for them is the figure of AMD's public "AMD Instinct MI300 (CDNA3)
Instruction Set Architecture Reference Guide", chapter "Instructions", section "VOP1 Instructions",
entries V_EXP_F32, V_LOG_F32 and V_RSQ_F32 (each reads "1ULP accuracy"; the Vega and GCN3 ISA guides
carry the same entries). That document is not part of a ROCm installation, so the figure cannot
be checked from the tree; it is named here so that it can be. The terms used:
  * exp:  rel. error 2u|x| (the rounded constant and the product, amplified by the exponent)
          + 2u (1 ulp = 2**-23 relative), plus 2**-126 absolute (denormal results flush);
  * log:  abs. error 2 * 2u * max(1, |log s|): 1 ulp of v_log_f32 taken at a result magnitude of
          at least 1 (s is in [1, J]), once more for the multiplication by ln 2. Near s = 1 this
          floor of 4u (2.4e-7) is looser than 1 ulp of the result; it is kept because the header
          only names ``__builtin_logf``, whose expansion around 1 is not documented;
  * rsqrt: rel. error 2u.
"""
import pytest
import torch
import torch.nn.functional as F

from exactness import BF16_EPS as b_, FP32_EPS as u_, assert_within, gauss_bf16

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
NHWC = ("n", "h", "w", "c")
EPS = float(torch.tensor(1e-5, dtype=torch.float32))  # the float the kernels receive


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _dev_nhwc(t):
    return _nhwc(t).to(BF16).to(DEV)


def _cv(v):
    return v.view(1, -1, 1, 1)


# ------------------------------------------------------------------ BatchNorm bounds
def bn_fwd_terms(z, gamma, beta, res=None):
    """fp64 BatchNorm of NCHW z with its own batch statistics, and the error terms of the
    kernels' fp32 evaluation (bn_act.hip finalize_fwd_ch / fold_fwd_coeffs, apply expression
    ``bf2f(z) * sc + sh (+ res)``; linear_ce.hip repeats both for the fused head).

    | quantity                        | roundings                                   | term          |
    |---------------------------------|---------------------------------------------|---------------|
    | stats S1, S2 (kernel inputs)    | stored as fp32: 1 each                      |               |
    | mu = S1 / M                     | input + division: 2                         | dmu = 2u|mu|  |
    | var = S2 / M - mu * mu          | 2 on S2/M, 5 on mu*mu (4 + product), 1 sub  | dv            |
    | is = rsqrtf(var + eps)          | dv / (var + eps) and the add, halved; 1 ulp | ris           |
    | sc = gamma * is                 | 1                                           | rsc = ris + u |
    | sh = beta - mu * sc             | product, subtraction                        | in dy         |
    | y = z * sc + sh (+ res)         | product, add (, add)                        | in dy         |

    y depends on sc through (z - mu) * sc, so the relative error of sc multiplies |(z - mu) sc|,
    not |z sc| + |mu sc| (the two share the same sc)."""
    C = z.shape[1]
    M = z.numel() // C
    S1, S2 = z.sum((0, 2, 3)), (z * z).sum((0, 2, 3))
    mu = S1 / M
    var = (S2 / M - mu * mu).clamp_min(0.0)
    ve = var + EPS
    is_ = ve.rsqrt()
    g, be = gamma.double(), beta.double()
    sc = g * is_
    sh = be - mu * sc
    dv = u_ * (2 * S2 / M + 5 * mu * mu + var)
    ris = 0.5 * (dv / ve + u_) + 2 * u_
    rsc = ris + u_
    dmu = 2 * u_ * mu.abs()
    y0 = z * _cv(sc) + _cv(sh)
    y = y0 if res is None else y0 + res
    dy = (((z - _cv(mu)) * _cv(sc)).abs() * _cv(rsc) + _cv(sc.abs() * dmu)
          + (1 + _cv(rsc)) * u_ * ((z * _cv(sc)).abs() + _cv(2 * (mu * sc).abs() + sh.abs())
                                   + y0.abs() + y.abs()))
    xh = (z - _cv(mu)) * _cv(is_)
    dxh = _cv(is_) * (_cv(dmu) + u_ * (z - _cv(mu)).abs()) + xh.abs() * _cv(ris + u_)
    stats = torch.zeros(16, 2 * C)
    stats[3] = torch.cat([S1, S2]).float()  # one of the 16 replicas, rounded to fp32
    return dict(M=M, mu=mu, is_=is_, sc=sc, sh=sh, rsc=rsc, ris=ris, y=y, dy=dy, xh=xh, dxh=dxh,
                stats=stats, gamma=g)


def bn_out_bound(t, relu, pool):
    """Reference output and its bound: ReLU and max are 1-Lipschitz, so the pre-activation's
    error bound passes through (the window's largest one for a pooled value); one bf16 store."""
    a = F.relu(t["y"]) if relu else t["y"]
    d = t["dy"]
    if pool:
        a, d = F.max_pool2d(a, 2, 2), F.max_pool2d(d, 2, 2)
    return a, b_ * a.abs() + (1 + b_) * d


def bn_undecidable(t, relu, pool):
    """Elements whose backward branch the fp64 reference cannot decide: a ReLU input within its
    bound of 0; a pool window whose two largest values come from different z and are closer than
    their bounds (equal z of one channel give equal y in the kernel and in the reference: both
    take the first). A window is undecidable as a whole."""
    y, dy = t["y"], t["dy"]
    ex = (y.abs() <= dy) if relu else torch.zeros_like(y, dtype=torch.bool)
    if pool:
        N, C, H, W = y.shape
        a = F.relu(y) if relu else y
        win = lambda v: v.reshape(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(
            N, C, H // 2, W // 2, 4)
        aw, dw, zw, ew = win(a), win(dy), win(t["z"]), win(ex)
        top = aw.max(-1, keepdim=True)
        arg = aw.argmax(-1, keepdim=True)
        near = (top.values - aw <= dw + dw.gather(-1, arg)) & (zw != zw.gather(-1, arg))
        near &= (top.values > 0) | (not relu)  # all-negative windows: every gradient is 0
        near &= _cv(t["gamma"] != 0).unsqueeze(-1)
        bad = (near.any(-1) | ew.any(-1))
        ex = bad.repeat_interleave(2, -2).repeat_interleave(2, -1)
    return ex


def bn_bwd_bounds(t, dyb, ddyb, ex):
    """fp64 dz, dgamma, dbeta for the gradient ``dyb`` at the BatchNorm output (already routed and
    masked by the reference) known to the kernel within ``ddyb``, with their bounds (bn_act.hip
    reduce / finalize / apply and the local kernel, conv_igemm.hip bnbwd_from_dx):

    | quantity                               | roundings                          |
    |----------------------------------------|------------------------------------|
    | xhat = (z - mu) * is                   | dmu, 1 sub, ris, 1 product  -> dxh |
    | S1 = sum dyb (M terms, any order)      | M                                  |
    | S2 = sum dyb * xhat                    | M + 1 (the product)                |
    | k = S * inv_m, inv_m = 1 / M           | 2                                  |
    | dgamma / dbeta: 16 replicas, +=        | 16                                 |
    | inner = dyb - k1 - xhat * k2           | 1 product, 2 subtractions          |
    | dz = sc * inner                        | rsc, 1 product; then one bf16 store|

    Undecidable elements (``ex``) may move their gradient: the channel sums get that much slack."""
    M = t["M"]
    xh, dxh = t["xh"], t["dxh"]
    sm = lambda v: v.sum((0, 2, 3))
    slack1 = sm(torch.where(ex, dyb.abs() + ddyb, torch.zeros_like(dyb)))
    slack2 = sm(torch.where(ex, (dyb.abs() + ddyb) * 2 * xh.abs(), torch.zeros_like(dyb)))
    S1, S2 = sm(dyb), sm(dyb * xh)
    dS1 = sm(ddyb) + M * u_ * sm(dyb.abs()) + slack1
    dS2 = sm(ddyb * xh.abs() + dyb.abs() * dxh) + (M + 1) * u_ * sm((dyb * xh).abs()) + slack2
    k1, k2 = S1 / M, S2 / M
    dk1, dk2 = dS1 / M + 2 * u_ * k1.abs(), dS2 / M + 2 * u_ * k2.abs()
    inner = dyb - _cv(k1) - xh * _cv(k2)
    din = (ddyb + _cv(dk1) + _cv(k2.abs()) * dxh + xh.abs() * _cv(dk2)
           + u_ * ((xh * _cv(k2)).abs() + (dyb - _cv(k1)).abs() + inner.abs()))
    dz = _cv(t["sc"]) * inner
    ddz = _cv(t["sc"].abs()) * din + dz.abs() * _cv(t["rsc"] + u_)
    return dict(dz=dz, dz_bound=b_ * dz.abs() + (1 + b_) * ddz,
                dgamma=S2, dgamma_bound=dS2 + 16 * u_ * S2.abs(),
                dbeta=S1, dbeta_bound=dS1 + 16 * u_ * S1.abs())


def _bn_inputs(N, C, H, res, seed):
    """z = 2 randn + 0.5 (bf16-valued); gamma of mixed sign, exactly 0 on two channels; one
    channel of constant z (variance 0)."""
    z = gauss_bf16((N, C, H, H), seed, 2.0, 0.5).double()
    z[:, 5] = 0.5
    g = torch.Generator().manual_seed(seed + 1)
    gamma = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
    gamma[2] = 0.0
    gamma[C - 3] = 0.0
    assert bool((gamma > 0).any()) and bool((gamma < 0).any())
    beta = torch.randn(C, generator=g) * 0.1
    r = gauss_bf16((N, C, H, H), seed + 2).double() if res else None
    return z, gamma.float(), beta.float(), r


BN_SHAPES = [(8, 64, 8, True, False), (8, 128, 4, False, False), (8, 512, 2, True, False),
             (8, 256, 8, False, True), (3, 64, 6, True, False), (5, 72, 3, False, False)]


BN_CASES = [(*sh, m) for sh in BN_SHAPES for m in ("split", "local", "mask", "mask-local")]


@pytest.mark.parametrize("N,C,H,pool,res,mode", BN_CASES)
def test_bn_act_per_element(native_ext, N, C, H, pool, res, mode):
    """out, dz, dres per element and each channel's dgamma / dbeta, in the reduce -> finalize ->
    apply chain (split), the one-block local kernel, and (mask, mask-local) with the forward
    storing the ReLU mask bits and the backward reading them in place of the residual.
    (3, 64, 6) and (5, 72, 3) leave partial item blocks; C = 72 gives 9 mask bytes per pixel.

    Refusals (``invalid arguments``, nothing written): a mask together with pooling, in the
    forward and in the backward (bn_act.hip ddp_bn_act_fwd / ddp_bn_act_bwd: the mask serves
    the unpooled kernels, with or without a residual); C = 72 in the reduce chain, whose 9
    channel groups do not tile its 256 threads -- the forward and the local kernel take it."""
    from ddp_amd.ops.common import ptr, stream_handle
    nat = native_ext
    use_mask = mode.startswith("mask")
    local = mode.endswith("local")
    z, gamma, beta, r = _bn_inputs(N, C, H, res, 100 + C + H)
    t = bn_fwd_terms(z, gamma, beta, r)
    t["z"] = z
    out_ref, out_bound = bn_out_bound(t, True, pool)
    ex = bn_undecidable(t, True, pool)
    # the reference's own routing and mask, through autograd of the same fp64 expression
    yl = t["y"].clone().requires_grad_(True)
    a = F.relu(yl)
    a = F.max_pool2d(a, 2, 2) if pool else a
    dout = gauss_bf16(tuple(a.shape), 300 + C).double()
    a.backward(dout)
    dyb = yl.grad
    bw = bn_bwd_bounds(t, dyb, torch.zeros_like(dyb), ex)

    zn, rn = _dev_nhwc(z), (_dev_nhwc(r) if res else None)
    gd, bd, sd = gamma.to(DEV), beta.to(DEV), t["stats"].to(DEV)
    doutn = _dev_nhwc(dout)
    Ho = H // 2 if pool else H
    out = torch.full((N, Ho, Ho, C), float("nan"), device=DEV, dtype=BF16)
    coef = torch.full((6 * C,), float("nan"), device=DEV)
    mask = torch.full((N, H, H, C // 8), 0xA5, dtype=torch.uint8, device=DEV) if use_mask else None
    sums = torch.zeros(16 * 2 * C, device=DEV)
    dz = torch.full((N, H, H, C), float("nan"), device=DEV, dtype=BF16)
    dres = torch.full((N, H, H, C), float("nan"), device=DEV, dtype=BF16) if res else None
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    s = stream_handle()

    def fwd():
        nat.bn_act_fwd(N, H, H, C, int(pool), 1, EPS, ptr(zn), ptr(rn), ptr(sd), ptr(gd), ptr(bd),
                       ptr(out), s, coef=ptr(coef), mask=ptr(mask))

    def bwd():  # with the mask bits the residual is not passed: the bits stand in for it
        nat.bn_act_bwd(N, H, H, C, int(pool), 1, EPS, ptr(zn), 0 if use_mask else ptr(rn),
                       ptr(sd), ptr(gd), ptr(bd), ptr(doutn), ptr(sums), ptr(dz), ptr(dres),
                       ptr(dg), ptr(db), 0, s, ptr(coef), mask=ptr(mask))

    def nothing_written_by_bwd():
        return (bool(torch.isnan(dz.float()).all()) and float(dg.abs().sum()) == 0.0
                and float(db.abs().sum()) == 0.0 and float(sums.abs().sum()) == 0.0
                and (dres is None or bool(torch.isnan(dres.float()).all())))

    if use_mask and pool:
        nat.bn_bwd_local_set(64 if local else 0)
        try:
            with pytest.raises(RuntimeError, match="invalid arguments"):
                fwd()
            with pytest.raises(RuntimeError, match="invalid arguments"):
                bwd()
            torch.cuda.synchronize()
        finally:
            nat.bn_bwd_local_set(8)
        assert bool(torch.isnan(out.float()).all()) and bool(torch.isnan(coef).all())
        assert bool((mask == 0xA5).all()) and nothing_written_by_bwd()
        return
    fwd()
    torch.cuda.synchronize()
    print("out", assert_within(out, _nhwc(out_ref), _nhwc(out_bound), NHWC, what="out"))
    if use_mask:  # bit e of a byte = (y > 0) of channel 8 * byte + e, wherever the sign is decided
        bits = ((mask.cpu().long().unsqueeze(-1) >> torch.arange(8)) & 1).reshape(N, H, H, C)
        want = _nhwc(t["y"] > 0).long()
        keep = ~_nhwc(ex)
        assert float(_nhwc(ex).double().mean()) <= 0.005
        assert torch.equal(bits[keep], want[keep]), "ReLU mask bits"

    refused = not local and (256 % (C // 8)) != 0
    nat.bn_bwd_local_set(64 if local else 0)
    try:
        assert bool(nat.bn_bwd_local_ok(N, H, H, C, int(pool))) == local
        if refused:
            with pytest.raises(RuntimeError, match="invalid arguments"):
                bwd()
        else:
            bwd()
        torch.cuda.synchronize()
    finally:
        nat.bn_bwd_local_set(8)
    if refused:
        assert nothing_written_by_bwd()
        return
    print("dz", assert_within(dz, _nhwc(bw["dz"]), _nhwc(bw["dz_bound"]), NHWC, _nhwc(ex),
                              what="dz"))
    if res:  # dres = dy_bn, a bf16 value passed through: equal wherever the branch is decidable
        assert_within(dres, _nhwc(dyb), 0.0, NHWC, _nhwc(ex), what="dres")
    print("dgamma", assert_within(dg, bw["dgamma"], bw["dgamma_bound"], ("c",), what="dgamma"))
    print("dbeta", assert_within(db, bw["dbeta"], bw["dbeta_bound"], ("c",), what="dbeta"))


# ------------------------------------------------------------------ softmax cross-entropy
def _rexp(x):
    """Relative error of __expf at argument x (see the module docstring)."""
    return 2 * u_ * x.abs() + 2 * u_ + u_


def ce_bounds(logits, labels, dl_in, n_sum, out_bf16):
    """fp64 mean cross-entropy of [B][J] ``logits`` (known to the kernel within ``dl_in``) and
    dlogits = (softmax - onehot) / B with their bounds (linear_ce.hip softmax_ce_kernel and the
    tail of linear_ce_fwd_kernel):

    | quantity                              | roundings                                        |
    |---------------------------------------|--------------------------------------------------|
    | x_j = l_j - mx                        | 1 sub, dl_in twice                               |
    | e_j = __expf(x_j)                     | _rexp(x_j), |x_j| error amplified by e_j         |
    | se = sum e_j (n_sum terms, any order) | n_sum                                            |
    | lse = mx + __logf(se)                 | rel. error of se, the log term, 1 add            |
    | p_j = __expf(l_j - lse)               | error of the argument (abs) + _rexp              |
    | d_j = (p_j - onehot) * inv_b          | 1 sub, inv_b, 1 product: 3 (+ one bf16 store)    |
    | loss = sum_b (lse - l_y) * inv_b      | 1 sub, 2; B atomic additions                     |
    """
    B, J = logits.shape
    mx = logits.max(1, keepdim=True).values
    x = logits - mx
    e = x.exp()
    se = e.sum(1, keepdim=True)
    dx = 2 * dl_in.max(1, keepdim=True).values + u_ * x.abs()
    dse = (e * (dx + _rexp(x))).sum(1, keepdim=True) + n_sum * u_ * se
    lg = se.log()
    lse = mx + lg
    dlse = (dl_in.max(1, keepdim=True).values + dse / se + 4 * u_ * lg.abs().clamp_min(1.0)
            + u_ * lse.abs())
    xa = logits - lse
    p = xa.exp()
    dp = p * (dl_in + dlse + u_ * xa.abs() + _rexp(xa)) + 2.0 ** -126
    oh = F.one_hot(labels, J).double()
    d = (p - oh) / B
    dd = dp / B + 3 * u_ * d.abs()
    d_bound = b_ * d.abs() + (1 + b_) * dd if out_bf16 else dd
    ly = logits.gather(1, labels.view(-1, 1))
    terms = (lse - ly) / B
    dly = dl_in.gather(1, labels.view(-1, 1))
    loss = terms.sum()
    loss_bound = ((dlse + dly + u_ * (lse - ly).abs()) / B + 2 * u_ * terms.abs()).sum() \
        + B * u_ * terms.abs().sum()
    return loss, loss_bound, d, d_bound


ROW_KINDS = ["plain_first", "plus80", "minus80", "tie", "plain_last"]


def _ce_row(kind, J, seed):
    g = torch.Generator().manual_seed(seed)
    row = torch.randn(J, generator=g) * 3
    if kind == "plus80":
        row += 80
    if kind == "minus80":
        row -= 80
    row = row.to(BF16).double()
    label = J - 1 if kind == "plain_last" else 0
    if kind == "tie" and J > 1:  # the two largest exactly equal, the label at the later one
        i, k = sorted(torch.topk(row, 2).indices.tolist())
        row[i] = row[k] = row.max()
        label = k
    return row, label


@pytest.mark.parametrize("out_bf16", [0, 1])
@pytest.mark.parametrize("in_bf16", [0, 1])
@pytest.mark.parametrize("J", [1, 10, 255, 256, 257, 1000])
@pytest.mark.parametrize("B", [1, 5])
def test_softmax_ce_per_element(native_ext, B, J, in_bf16, out_bf16):
    """Loss, correct and every dlogits element, fp32 / bf16 logits and dlogits, labels at 0 and
    J - 1, rows at +80 and -80, a row whose two largest logits are equal (``correct`` follows
    the lowest index, so the label at the later one is a miss). B = 1 takes each row kind alone."""
    from ddp_amd.ops.common import ptr, stream_handle
    batches = [ROW_KINDS] if B == 5 else [[k] for k in ROW_KINDS]
    for kinds in batches:
        rows = [_ce_row(k, J, 400 + J + i) for i, k in enumerate(kinds)]
        logits = torch.stack([r for r, _ in rows])
        labels = torch.tensor([l for _, l in rows], dtype=torch.int64)
        ld = logits.to(BF16 if in_bf16 else torch.float32).to(DEV)
        loss = torch.zeros((), device=DEV)
        correct = torch.zeros((), dtype=torch.int32, device=DEV)
        dl = torch.full((B, J), float("nan"), device=DEV,
                        dtype=BF16 if out_bf16 else torch.float32)
        native_ext.softmax_ce(ptr(ld), in_bf16, ptr(labels.to(DEV)), B, J, ptr(loss), ptr(correct),
                              ptr(dl), out_bf16, stream_handle())
        torch.cuda.synchronize()
        want_loss, loss_bound, d, d_bound = ce_bounds(logits, labels, torch.zeros_like(logits), J,
                                                      out_bf16)
        assert torch.allclose(want_loss, F.cross_entropy(logits, labels), rtol=1e-12, atol=1e-12)
        # argmax with the lowest index among equals
        first = torch.tensor([int(torch.nonzero(r == r.max())[0]) for r in logits])
        assert int(correct) == int((first == labels).sum()), kinds
        assert_within(loss.cpu().double().view(1), want_loss.view(1), loss_bound.view(1),
                      what=f"loss {kinds}")
        assert_within(dl, d, d_bound, ("b", "j"), what=f"dlogits {kinds}")
        # each row of the true gradient sums to 0: the kernel's row sums stay within the bounds
        assert_within(dl.double().sum(1).cpu(), torch.zeros(B, dtype=torch.float64),
                      d_bound.sum(1), ("b",), what=f"row sums {kinds}")


# ------------------------------------------------------------------ fused head
def _head_inputs(B, Fi, J, seed):
    z, gamma, beta, _ = _bn_inputs(B, Fi, 2, False, seed)
    g = torch.Generator().manual_seed(seed + 7)
    W = (torch.randn(J, Fi, generator=g) * 0.05).float()
    bias = (torch.randn(J, generator=g) * 0.1).float()
    labels = torch.randint(0, J, (B,), generator=g)
    labels[0], labels[-1] = 0, J - 1
    return z, gamma, beta, W, bias, labels


def _logit_terms(x64, W, bias):
    """fp64 logits of the stored bf16 features and their bound: F products and additions in any
    order plus the bias (linear_ce_fwd_kernel acc / wave_sum): (F + 1) u T."""
    Wd, bd = W.double(), bias.double()
    logits = x64 @ Wd.t() + bd
    T = x64.abs() @ Wd.abs().t() + bd.abs()
    return logits, (x64.shape[1] + 1) * u_ * T


@pytest.mark.parametrize("Fi", [64, 512, 1024])
@pytest.mark.parametrize("B", [3, 32])
def test_fused_head_forward(native_ext, B, Fi):
    """bn_pool_linear_ce_fwd against bn_act_fwd (pool) + linear_ce_fwd on the same z and
    statistics: the stored bf16 features and the coefficient table bit for bit (same apply
    expression, same pool rule), loss and dlogits per element against fp64 on those features."""
    from ddp_amd.ops.common import ptr, stream_handle
    nat = native_ext
    J = 10
    z, gamma, beta, W, bias, labels = _head_inputs(B, Fi, J, 500 + Fi)
    t = bn_fwd_terms(z, gamma, beta)
    zn = _dev_nhwc(z)
    gd, bd, sd = gamma.to(DEV), beta.to(DEV), t["stats"].to(DEV)
    Wd, biasd, yd = W.to(DEV), bias.to(DEV), labels.to(DEV)
    s = stream_handle()
    x_sep = torch.full((B, 1, 1, Fi), float("nan"), device=DEV, dtype=BF16)
    coef_sep = torch.full((6 * Fi,), float("nan"), device=DEV)
    nat.bn_act_fwd(B, 2, 2, Fi, 1, 1, EPS, ptr(zn), 0, ptr(sd), ptr(gd), ptr(bd), ptr(x_sep), s,
                   coef=ptr(coef_sep))
    dl_sep = torch.full((B, J), float("nan"), device=DEV)
    loss_sep = torch.zeros((), device=DEV)
    nat.linear_ce_fwd(ptr(x_sep), ptr(Wd), ptr(biasd), ptr(yd), B, Fi, J, 0, ptr(dl_sep),
                      ptr(loss_sep), 0, s)
    x = torch.full((B, Fi), float("nan"), device=DEV, dtype=BF16)
    coef = torch.full((6 * Fi,), float("nan"), device=DEV)
    dl = torch.full((B, J), float("nan"), device=DEV)
    loss = torch.zeros((), device=DEV)
    nat.bn_pool_linear_ce_fwd(ptr(zn), ptr(sd), ptr(gd), ptr(bd), EPS, 1, ptr(coef), ptr(x),
                              ptr(Wd), ptr(biasd), ptr(yd), B, Fi, J, ptr(dl), ptr(loss), s)
    torch.cuda.synchronize()
    assert torch.equal(x.view(torch.int16), x_sep.view(B, Fi).view(torch.int16)), "features"
    # the fused head writes the forward rows sc, sh, mu, is (linear_ce.hip); rows 4 and 5 (k1, k2)
    # belong to the backward and must be left alone by both paths
    assert torch.equal(coef[:4 * Fi].view(torch.int32), coef_sep[:4 * Fi].view(torch.int32)), "coef"
    assert bool(torch.isnan(coef[4 * Fi:]).all()) and bool(torch.isnan(coef_sep[4 * Fi:]).all())
    # the features themselves, per element, against the fp64 BatchNorm + ReLU + pool
    out_ref, out_bound = bn_out_bound(t, True, True)
    assert_within(x.view(B, 1, 1, Fi), _nhwc(out_ref), _nhwc(out_bound), NHWC, what="features")
    logits, dlog = _logit_terms(x.double().cpu(), W, bias)
    want_loss, loss_bound, d, d_bound = ce_bounds(logits, labels, dlog, J, 0)
    for name, got_l, got_d in (("fused", loss, dl), ("separate", loss_sep, dl_sep)):
        assert_within(got_l.cpu().double().view(1), want_loss.view(1), loss_bound.view(1),
                      what=name + " loss")
        assert_within(got_d, d, d_bound, ("b", "j"), what=name + " dlogits")


def test_fused_head_refuses_wide_features(native_ext):
    """F = 1032 > kMaxHeadF: the coefficient table would not fit the block's LDS."""
    from ddp_amd.ops.common import ptr, stream_handle
    B, Fi, J = 3, 1032, 10
    zn = torch.zeros(B, 2, 2, Fi, device=DEV, dtype=BF16)
    st = torch.zeros(16, 2 * Fi, device=DEV)
    v = torch.ones(Fi, device=DEV)
    coef = torch.full((6 * Fi,), float("nan"), device=DEV)
    x = torch.full((B, Fi), float("nan"), device=DEV, dtype=BF16)
    W, bias = torch.zeros(J, Fi, device=DEV), torch.zeros(J, device=DEV)
    y = torch.zeros(B, dtype=torch.int64, device=DEV)
    dl = torch.full((B, J), float("nan"), device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    with pytest.raises(RuntimeError, match="invalid arguments"):
        native_ext.bn_pool_linear_ce_fwd(ptr(zn), ptr(st), ptr(v), ptr(v), EPS, 1, ptr(coef), ptr(x),
                                         ptr(W), ptr(bias), ptr(y), B, Fi, J, ptr(dl), ptr(loss),
                                         stream_handle())
    torch.cuda.synchronize()
    for tns in (coef, x, dl, loss):
        assert bool(torch.isnan(tns.float()).all())


@pytest.mark.parametrize("Fi", [64, 512, 1024])
@pytest.mark.parametrize("B", [3, 32])
def test_fused_head_backward(native_ext, B, Fi):
    """linear_head_bwd_bn (dx never stored, the block's whole BatchNorm backward, dW and db in
    one launch) and linear_bwd + bn_act_bwd on the same inputs, each per element against fp64:
    dW, db, dz and the block's dgamma / dbeta.

    dx = (g dl) W is consumed as bf16 by both paths (linear_ce.hip linear_dx_block f2bf;
    conv_igemm.hip bnbwd_from_dx round_bf), so the gradient at the BatchNorm output is known to
    the kernels within b |dx| + (J + 1) u sum_j |g dl_j W_jf| (dl * g, J products and additions).
    dW = g sum_b dl x: B products and additions in 8-row chunks met by atomics, times g:
    (B + 2) u T; db the same without the product."""
    from ddp_amd.ops.common import ptr, stream_handle
    nat = native_ext
    J, gs = 10, 2.0
    z, gamma, beta, W, bias, labels = _head_inputs(B, Fi, J, 600 + Fi)
    t = bn_fwd_terms(z, gamma, beta)
    t["z"] = z
    zn = _dev_nhwc(z)
    gd, bd, sd = gamma.to(DEV), beta.to(DEV), t["stats"].to(DEV)
    Wd, biasd, yd = W.to(DEV), bias.to(DEV), labels.to(DEV)
    s = stream_handle()
    x = torch.full((B, 1, 1, Fi), float("nan"), device=DEV, dtype=BF16)
    coef = torch.full((6 * Fi,), float("nan"), device=DEV)
    nat.bn_act_fwd(B, 2, 2, Fi, 1, 1, EPS, ptr(zn), 0, ptr(sd), ptr(gd), ptr(bd), ptr(x), s,
                   coef=ptr(coef))
    dl = torch.full((B, J), float("nan"), device=DEV)
    nat.linear_ce_fwd(ptr(x), ptr(Wd), ptr(biasd), ptr(yd), B, Fi, J, 0, ptr(dl), 0, 0, s)
    g = torch.tensor([gs], device=DEV)
    # separate: head backward, then the block's BatchNorm backward on the stored dx
    dx = torch.full((B, 1, 1, Fi), float("nan"), device=DEV, dtype=BF16)
    dW_a, db_a = torch.zeros(J, Fi, device=DEV), torch.zeros(J, device=DEV)
    nat.linear_bwd(ptr(dl), ptr(x), ptr(Wd), B, Fi, J, ptr(g), ptr(dx), ptr(dW_a), ptr(db_a), s)
    sums_a = torch.zeros(16 * 2 * Fi, device=DEV)
    dz_a = torch.full((B, 2, 2, Fi), float("nan"), device=DEV, dtype=BF16)
    dg_a, dbt_a = torch.zeros(Fi, device=DEV), torch.zeros(Fi, device=DEV)
    nat.bn_act_bwd(B, 2, 2, Fi, 1, 1, EPS, ptr(zn), 0, ptr(sd), ptr(gd), ptr(bd), ptr(dx),
                   ptr(sums_a), ptr(dz_a), 0, ptr(dg_a), ptr(dbt_a), 0, s, ptr(coef))
    # fused
    sums_b = torch.zeros(16 * 2 * Fi, device=DEV)
    dz_b = torch.full((B, 2, 2, Fi), float("nan"), device=DEV, dtype=BF16)
    dg_b, dbt_b = torch.zeros(Fi, device=DEV), torch.zeros(Fi, device=DEV)
    dW_b, db_b = torch.zeros(J, Fi, device=DEV), torch.zeros(J, device=DEV)
    served = nat.linear_head_bwd_bn(ptr(dl), ptr(Wd), ptr(x), B, Fi, J, ptr(g),
                                    (ptr(zn), ptr(coef), ptr(sums_b), 1, 1, 2, 2),
                                    (ptr(dz_b), ptr(dg_b), ptr(dbt_b)), ptr(dW_b), ptr(db_b), s)
    torch.cuda.synchronize()
    assert served
    # fp64 reference from the kernels' own inputs: dl (fp32), the stored features x, z
    dl64, x64, W64 = dl.double().cpu() * gs, x.view(B, Fi).double().cpu(), W.double()
    dW_ref, dW_T = dl64.t() @ x64, dl64.abs().t() @ x64.abs()
    db_ref, db_T = dl64.sum(0), dl64.abs().sum(0)
    dx_ref, dx_T = dl64 @ W64, dl64.abs() @ W64.abs()
    ddx = b_ * dx_ref.abs() + (1 + b_) * (J + 1) * u_ * dx_T
    # route dx through the reference's pool and ReLU
    yl = t["y"].clone().requires_grad_(True)
    F.max_pool2d(F.relu(yl), 2, 2).backward(dx_ref.view(B, Fi, 1, 1))
    dyb = yl.grad
    ddyb = torch.where(dyb != 0, ddx.view(B, Fi, 1, 1).expand_as(dyb), torch.zeros_like(dyb))
    ex = bn_undecidable(t, True, True)
    bw = bn_bwd_bounds(t, dyb, ddyb, ex)
    for name, dW, db, dz, dg, dbt in (("separate", dW_a, db_a, dz_a, dg_a, dbt_a),
                                      ("fused", dW_b, db_b, dz_b, dg_b, dbt_b)):
        assert_within(dW, dW_ref, (B + 2) * u_ * dW_T, ("j", "f"), what=name + " dW")
        assert_within(db, db_ref, (B + 2) * u_ * db_T, ("j",), what=name + " db")
        assert_within(dz, _nhwc(bw["dz"]), _nhwc(bw["dz_bound"]), NHWC, _nhwc(ex),
                      what=name + " dz")
        assert_within(dg, bw["dgamma"], bw["dgamma_bound"], ("c",), what=name + " dgamma")
        assert_within(dbt, bw["dbeta"], bw["dbeta_bound"], ("c",), what=name + " dbeta")
