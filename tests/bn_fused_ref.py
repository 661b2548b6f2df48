"""fp64 reference of the BatchNorm backward that conv_igemm.hip fuses into DGRAD epilogues and
split-K finishes (BnBwdFuse / BnBwdApply), from a GIVEN coefficient table; importable without a GPU.

Every fused site reads the preceding block's scale, shift, mean and invstd from rows 0-3 of the
table coef[6][C]; a test passes the table in, so it can write it with powers of two:

  z in {-4..4}, scale in {1, -1, .5, -.5, 2, 0}, shift in {-2, -1, 0, .5, 1},
  mean in {-1, 0, .5, 1}, invstd in {.5, 1, 2}; dx = an exact integer DGRAD output.

Then y = z * sc + sh, xhat = (z - mu) * is and dy_bn * xhat are exact in fp32 (with or without FMA
contraction), S1 = sum dy_bn and S2 = sum dy_bn * xhat are multiples of ``UNIT`` far below 2**24
and so exact in any summation order, and where M (the element count per channel of z) is a power
of two so are k1 = S1 / M, k2 = S2 / M and dz = sc * (dy_bn - k1 - xhat * k2) before its bf16
store. ``bn_bwd_ref`` asserts that on the reference alone (``representable``), before any kernel
output is looked at. The kernel must then agree bit for bit.

Routing rule (bn_act.hip bwd_compute, which every fused site states it repeats): a pooled
gradient goes to the FIRST maximum of relu(y) in row-major window order d = 2r + c, the ReLU
gradient is 0 at y <= 0. That is F.max_pool2d's / F.relu's autograd rule in fp64, which the
reference uses; ``bn_bwd_routed`` is the same computation with the routing spelled out, so that a
wrong rule (last maximum, a neighbouring pixel, ...) can be put in its place: test_bn_fused_ref_cpu
shows the two agree and that each such defect changes S1, S2 or dz.
"""
import torch
import torch.nn.functional as F

from exactness import BF16_EPS, FP32_EPS, coords, mismatches, int_tensor

BF16 = torch.bfloat16
SCALES = (1.0, -1.0, 0.5, -0.5, 2.0, 0.0)
SHIFTS = (-2.0, -1.0, 0.0, 0.5, 1.0)
MEANS = (-1.0, 0.0, 0.5, 1.0)
INVSTDS = (0.5, 1.0, 2.0)
# dy_bn is an integer, z - mean a multiple of 1/2, invstd at least 1/2: the sums are multiples of
UNIT = 0.5 * 0.5


def cv(v):
    return v.view(1, -1, 1, 1)


def win(v):
    """NCHW -> [N][C][H/2][W/2][4], window positions in bn_act.hip's order d = 2r + c."""
    N, C, H, W = v.shape
    return v.reshape(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(
        N, C, H // 2, W // 2, 4)


def unwin(v):
    N, C, Ho, Wo, _ = v.shape
    return v.reshape(N, C, Ho, Wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, 2 * Ho, 2 * Wo)


def coef_table(C, seed):
    """fp32 [6][C]: rows 0-3 drawn per channel from the power-of-two sets above (every scale
    value occurs once C >= 6: the draw is a seeded permutation of a repeated list), rows 4-5 (k1,
    k2 of the unfused backward; no fused site reads them) NaN."""
    g = torch.Generator().manual_seed(seed)
    t = torch.full((6, C), float("nan"))
    for row, vals in enumerate((SCALES, SHIFTS, MEANS, INVSTDS)):
        rep = torch.tensor(vals).repeat(C // len(vals) + 1)[:max(C, len(vals))]
        t[row] = rep[torch.randperm(rep.numel(), generator=g)][:C]
    return t


def z_tensor(N, C, Hz, Wz, seed):
    """NCHW integers in {-4..4} (fp64)."""
    return int_tensor((N, C, Hz, Wz), -4, 4, seed).double()


def representable(t):
    """Every element of the fp64 tensor is an fp32 number."""
    return bool((t.float().double() == t).all())


def _finish(dyb, z, coef, M, check):
    """S1, S2 and dz from the routed gradient dy_bn (z's shape), and ``dz_bound``: the bound of
    dz where M = Mg * NP is no power of two, counted from conv_igemm.hip bnbwd_from_dx (S1, S2,
    xhat and dy_bn are exact with these inputs; u = 2**-24, b = 2**-8):

    | quantity                          | roundings                          | source line          |
    |-----------------------------------|------------------------------------|----------------------|
    | inv_m = 1.f / ((float)Mg * NP)    | 1 (the product Mg * NP is exact)   | ``const float inv_m``|
    | k1 = S1 * inv_m                   | 1 more: 2u |k1|                    | ``k1[e] = S1 * inv_m``|
    | k2 = S2 * inv_m                   | 2u |k2|, times |xhat| in xhat * k2 | ``k2[e] = S2 * inv_m``|
    | xhat * k2                         | 1: u |xhat k2|                     | the ``o[e] =`` line  |
    | dy - k1                           | 1: u |dy - k1|                     |                      |
    | (dy - k1) - xhat * k2             | 1: u |inner|                       |                      |
    | sc * inner                        | 1: u |dz| (sc is a power of two)   |                      |
    | bf16 store                        | b |dz|                             | ``f2bf``             |

    din = 2u|k1| + 2u|xhat k2| + u(|xhat k2| + |dy - k1| + |inner|), ddz = |sc| din + u|dz|,
    bound = b |dz| + (1 + b) ddz. An FMA contraction removes roundings and stays inside."""
    sc, mu, is_ = (coef[i].double() for i in (0, 2, 3))
    xh = (z - cv(mu)) * cv(is_)
    sm = lambda v: v.sum((0, 2, 3))
    S1, S2 = sm(dyb), sm(dyb * xh)
    A1, A2 = sm(dyb.abs()), sm((dyb * xh).abs())
    k1, k2 = S1 / M, S2 / M
    t1 = dyb - cv(k1)
    t2 = xh * cv(k2)
    inner = t1 - t2
    dz = cv(sc) * inner
    pow2 = M & (M - 1) == 0
    if check:
        assert float(A1.max()) < 2 ** 24 and float(A2.max()) / UNIT < 2 ** 24
        assert representable(xh) and representable(dyb * xh)
        if pow2:  # every intermediate of dz: fix the inputs if this fails
            for name, t in (("k1", k1), ("k2", k2), ("dy - k1", t1), ("xhat * k2", t2),
                            ("inner", inner), ("dz", dz)):
                assert representable(t), f"{name} is not an fp32 number: choose other inputs"
    u = FP32_EPS
    din = 2 * u * cv(k1.abs()) + 2 * u * t2.abs() + u * (t2.abs() + t1.abs() + inner.abs())
    ddz = cv(sc.abs()) * din + u * dz.abs()
    return dict(dyb=dyb, xh=xh, S1=S1, S2=S2, A1=A1, A2=A2, k1=k1, k2=k2, dz=dz, M=M, pow2=pow2,
                dz_bound=BF16_EPS * dz.abs() + (1 + BF16_EPS) * ddz)


def bn_bwd_ref(dx64, z, coef, pool, relu, check=True):
    """The fused BN backward in fp64. ``dx64``: the exact DGRAD output, NCHW at the block output's
    resolution (it is rounded to bf16 here, like the stored / register dx of every fused site);
    ``z``: the block's conv output NCHW (twice the resolution when ``pool``); ``coef``: [>=4][C].
    Routing by autograd: y = z * sc + sh -> ReLU -> max_pool2d(2, 2), backward of bf16(dx)."""
    sc, sh = coef[0].double(), coef[1].double()
    dxb = dx64.to(BF16).double()
    zr = z.clone().requires_grad_(True)
    y = zr * cv(sc) + cv(sh)
    y.retain_grad()
    a = F.relu(y) if relu else y
    if pool:
        a = F.max_pool2d(a, 2, 2)
    assert a.shape == dxb.shape, (a.shape, dxb.shape)
    a.backward(dxb)
    N, C, Hz, Wz = z.shape
    r = _finish(y.grad.detach(), z, coef, N * Hz * Wz, check)
    r["dxb"] = dxb
    return r


def bn_bwd_routed(dx64, z, coef, pool, relu, tie="first", neighbour=None, drop_row=None,
                  m_factor=1):
    """The same computation with the routing explicit, and the defects a fused kernel could have:
    ``tie`` = "last": the last maximum of a window instead of the first; ``neighbour`` = (n, c, h,
    w): that window's gradient goes to the next pixel of its window; ``drop_row`` = flat NHW index
    of a dgrad row left out of the sums and of dz's dy; ``m_factor``: M divided by it (inv_m taken
    from the dgrad's rows instead of z's pixels)."""
    sc, sh = coef[0].double(), coef[1].double()
    dxb = dx64.to(BF16).double().clone()
    N, C, Hz, Wz = z.shape
    if drop_row is not None:
        H, W = dxb.shape[2:]
        n, rem = divmod(drop_row, H * W)
        dxb[n, :, rem // W, rem % W] = 0.0
    y = z * cv(sc) + cv(sh)
    yr = F.relu(y) if relu else y
    if pool:
        yw, ypre = win(yr), win(y)
        eq = yw == yw.max(-1, keepdim=True).values
        cs = eq.int().cumsum(-1)
        pick = eq & (cs == (1 if tie == "first" else cs[..., -1:]))
        pos = (pick.int() * torch.arange(4)).sum(-1, keepdim=True)
        if neighbour is not None:
            n, c, h, w = neighbour
            pos[n, c, h, w] = (pos[n, c, h, w] + 1) % 4
        ya = ypre.gather(-1, pos).squeeze(-1)
        d = torch.where(ya > 0, dxb, torch.zeros_like(dxb)) if relu else dxb
        dyb = unwin(torch.zeros_like(yw).scatter_(-1, pos, d.unsqueeze(-1)))
    else:
        dyb = torch.where(y > 0, dxb, torch.zeros_like(dxb)) if relu else dxb
    return _finish(dyb, z, coef, N * Hz * Wz // m_factor, False)


def canon_zero(t):
    """-0 -> +0 (x + 0 = +0 for both zeros in round to nearest), everything else unchanged."""
    return t + torch.zeros((), dtype=t.dtype)


def assert_dz_exact(got, ref64, names=None, what="dz", show=8):
    """``got`` (bf16) equals the bf16 image of the fp64 reference bit for bit, zeros compared
    without their sign. assert_exact demands +0 for an exact zero, because a sum onto a +0
    accumulator never gives -0; dz is a PRODUCT, sc * inner, and is rightly -0 where sc < 0 and
    inner is +0 or where sc is 0 and inner < 0. So both sides' zeros are taken as +0 here, and
    only here: S1, S2, dgamma, dbeta, dx and dw keep assert_exact's rule."""
    assert ref64.dtype == torch.float64 and got.dtype == BF16
    assert tuple(got.shape) == tuple(ref64.shape), (what, tuple(got.shape), tuple(ref64.shape))
    g = canon_zero(got.detach().cpu().contiguous())
    want = canon_zero(ref64.detach().cpu().to(BF16).contiguous())
    bad = mismatches(g, want).reshape(-1)
    nbad = int(bad.sum())
    if nbad == 0:
        return
    where = torch.nonzero(bad).reshape(-1)[:show].tolist()
    gf, wf = g.reshape(-1), want.reshape(-1)
    lab = lambda c: str(c) if names is None else "(" + ", ".join(
        f"{n}={v}" for n, v in zip(names, c)) + ")"
    lines = [f"  {lab(coords(i, g.shape))}: got {float(gf[i])!r} want {float(wf[i])!r}"
             for i in where]
    raise AssertionError(f"{what}: {nbad} of {bad.numel()} elements differ from the exact "
                         f"reference; first {len(where)}:\n" + "\n".join(lines))
