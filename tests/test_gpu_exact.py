"""Exact-mode tests of the kernels whose arithmetic is sums of products (tests/exactness.py).

Operands are integer-valued bf16 numbers: x, w in {-1, 0, 1}, bias in {-3..3}, dz in {-2..2}
(the head: {-2..2} throughout). Every product and partial sum is an integer far below 2**24, so
fp32 accumulation is exact in any order -- MFMA, split-K slabs, float atomics, LDS reductions --
and the kernel's output must EQUAL the fp64 reference (fp32 outputs) or its round-to-nearest-even
bf16 image (bf16 outputs; |z| may exceed 256 on the 512-channel layers and is then rounded, on
both sides alike). A wrong tile edge, a dropped tap or a lost reduction pixel changes an integer
and cannot hide. References are computed once per shape in fp64 on the CPU and never modified;
outputs are pre-filled with NaN (accumulated-onto ones with integers), so an unwritten element is
a mismatch.

Max-pool ties: integers in {-2..2} tie in more than half of the windows; the reference is
F.max_pool2d and its autograd in fp64 (first maximum in row-major window order), and every
window's gradient (positive integers, so nothing cancels) must reach exactly that one position.
"""
import pytest
import torch
import torch.nn.functional as F

from exactness import FP32_EPS, BF16_EPS, assert_exact, assert_within, int_tensor
from test_gpu_conv_index_math import SHAPES, TR_CASES as TR_DECLINE_CASES
from test_gpu_conv_tr import TR_CASES

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
NHWC = ("n", "h", "w", "c")
KCRS = ("k", "c", "r", "s")
_CACHE = {}


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _to_dev_nhwc(t, cpad=None):
    """NCHW fp32 integers (CPU) -> NHWC bf16 on the GPU, channels zero-padded to ``cpad``."""
    n = _nhwc(t).to(BF16)
    if cpad is not None and cpad != n.shape[-1]:
        p = torch.zeros(*n.shape[:-1], cpad, dtype=BF16)
        p[..., :n.shape[-1]] = n
        n = p
    return n.to(DEV)


def _conv_ref(x, w, b, dz, stride, pad, bwd):
    """fp64: z, dx (both NHWC), dw ([K][C][R][S]) and the channel sums of the rounded z."""
    x, w, dz = x.double(), w.double(), dz.double()
    z = _nhwc(F.conv2d(x, w, b.double(), stride, pad))
    zb = z.to(BF16).double().reshape(-1, z.shape[-1])
    r = dict(z=z, s1=zb.sum(0), s2=(zb * zb).sum(0), a1=zb.abs().sum(0))
    if bwd:
        xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        F.conv2d(xr, wr, None, stride, pad).backward(dz)
        r.update(dx=_nhwc(xr.grad), dw=wr.grad)
    return r


def _case(shape, creal=None, seed=7, bwd=True):
    """Integer operands of a conv shape (N, C, H, W, K, R, stride, pad) on the GPU, with the fp64
    references of FWD / DGRAD / WGRAD (``bwd`` = False: FWD only) and of the same operations on
    the magnitudes."""
    key = (shape, creal, seed, bwd)
    if key in _CACHE:
        return _CACHE[key]
    from ddp_amd.ops.layers import ConvBNActSpec
    N, C, H, W, K, R, stride, pad = shape
    Cr = creal or C
    P, Q = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    x = int_tensor((N, Cr, H, W), -1, 1, seed)
    w = int_tensor((K, Cr, R, R), -1, 1, seed + 1)
    b = int_tensor((K,), -3, 3, seed + 2)
    dz = int_tensor((N, K, P, Q), -2, 2, seed + 3)
    conv = torch.nn.Conv2d(Cr, K, R, stride, pad, bias=True).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    spec = ConvBNActSpec(conv, None, cin_pad=C)
    spec.maybe_pack()
    c = dict(conv=conv, spec=spec, xn=_to_dev_nhwc(x, C), dzn=_to_dev_nhwc(dz),
             ref=_conv_ref(x, w, b, dz, stride, pad, bwd),
             mag=_conv_ref(x.abs(), w.abs(), b.abs(), dz.abs(), stride, pad, bwd),
             dw0=int_tensor((K, Cr, R, R), -5, 5, seed + 4), P=P, Q=Q)
    _CACHE[key] = c
    return c


def _dw_start(c):
    """The integers WGRAD accumulates onto, in the arena's [K][R][S][C] memory order."""
    return c["dw0"].to(DEV).contiguous(memory_format=torch.channels_last)


def _check_stats(c, stats, K, what):
    st = stats.view(16, 2 * K).sum(0).cpu()
    assert_exact(st[:K], c["ref"]["s1"], c["ref"]["a1"], ("k",), what + " sum z")
    assert_exact(st[K:], c["ref"]["s2"], c["ref"]["s2"], ("k",), what + " sum z^2")
    # (the replicas themselves hold integers; their sum above is exact as well)


def _check_fwd(c, z, stats, K, what):
    assert_exact(z, c["ref"]["z"], c["mag"]["z"], NHWC, what + " z")
    if stats is not None:
        _check_stats(c, stats, K, what)


def _check_bwd(c, dx, dw, what):
    if dx is not None:
        assert_exact(dx[..., :c["ref"]["dx"].shape[-1]], c["ref"]["dx"], c["mag"]["dx"], NHWC,
                     what + " dx")
    if dw is not None:
        assert_exact(dw, c["ref"]["dw"] + c["dw0"].double(), c["mag"]["dw"] + c["dw0"].abs().double(),
                     KCRS, what + " dw")


# ------------------------------------------------------------------ conv GEMMs (conv_igemm.hip)
def _separate(nat, name, splits, rows_pm=None, wgrad_pm=None):
    """FWD, DGRAD and WGRAD as three launches with a forced split count, all exact."""
    from ddp_amd.ops.common import ptr, stream_handle, weight_krsc, workspace
    c = _case(SHAPES[name])
    N, C, H, W, K, R, stride, pad = SHAPES[name]
    spec, conv = c["spec"], c["conv"]
    ws, s = workspace(torch.device(DEV)), stream_handle()
    dw = _dw_start(c)
    g = spec.geom(N, H, W, weight_krsc(dw))
    z = torch.full((N, c["P"], c["Q"], K), float("nan"), device=DEV, dtype=BF16)
    dx = torch.full_like(c["xn"], float("nan"))
    stats = torch.zeros(16 * 2 * K, device=DEV)
    if rows_pm is not None:
        nat.conv_rows_pm_set(rows_pm)
    if wgrad_pm is not None:
        nat.conv_wgrad_pm_set(wgrad_pm)
    try:
        nat.conv_fwd(g, ptr(c["xn"]), ptr(spec.wc), ptr(conv.bias), ptr(z), ptr(stats), ptr(ws),
                     ws.numel(), splits, s)
        nat.conv_dgrad(g, ptr(c["dzn"]), ptr(spec.wc), ptr(dx), ptr(ws), ws.numel(), splits, s)
        nat.conv_wgrad(g, ptr(c["dzn"]), ptr(c["xn"]), ptr(dw), ptr(ws), ws.numel(), splits, s)
        torch.cuda.synchronize()
    finally:
        nat.conv_rows_pm_set(1)
        nat.conv_wgrad_pm_set(1)
    what = f"{name} splits {splits}"
    _check_fwd(c, z, stats, K, what)
    _check_bwd(c, dx, dw, what)


@pytest.mark.parametrize("splits", [1, 2, 3])
@pytest.mark.parametrize("tile", range(8))
@pytest.mark.parametrize("name", ["odd5x5", "pm4x4_n3", "corner16", "dense2x2", "s2_3x3", "s2_1x1",
                                  "s1_1x1"])
def test_every_tile_and_split_exact(native_ext, name, tile, splits):
    """z (integer bias included), the summed statistics replicas, dx and dw on every forced
    implicit-GEMM tile with 1-3 splits."""
    native_ext.conv_force_tile(tile + 1, 0)
    try:
        _separate(native_ext, name, splits)
    finally:
        native_ext.conv_force_tile(0, 0)


@pytest.mark.parametrize("splits", [1, 2, 3])
@pytest.mark.parametrize("rows_pm,wgrad_pm", [(0, 0), (1, 1), (2, 2)])
@pytest.mark.parametrize("name", ["pm4x4_n3", "pm4x4", "corner16", "corner16_n64"])
def test_pixel_major_on_and_off_exact(native_ext, name, rows_pm, wgrad_pm, splits):
    """Pixel-major rows / reduction off, on for small images and on for every image size, on the
    64x64 tile (the empty third split of a corner pixel must still write its zero slab)."""
    native_ext.conv_force_tile(4, 0)
    try:
        _separate(native_ext, name, splits, rows_pm, wgrad_pm)
    finally:
        native_ext.conv_force_tile(0, 0)


@pytest.mark.parametrize("sd,sw", [(1, 1), (2, 3), (3, 2), (3, 3)])
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("name", ["odd5x5", "pm4x4_n3", "pm4x4", "corner16", "dense2x2", "s1_1x1"])
def test_pair_every_tile_and_split_exact(native_ext, name, tile, sd, sw):
    """The backward pair (DGRAD + WGRAD in one launch) on every forced pair tile and split."""
    from ddp_amd.ops.layers import conv_backward
    c = _case(SHAPES[name])
    dw = _dw_start(c)
    native_ext.conv_pair_force(sd, sw, tile)
    try:
        dx = conv_backward(c["spec"], c["xn"], c["dzn"], dw, True)
        torch.cuda.synchronize()
    finally:
        native_ext.conv_pair_force(0, 0, 0)
    _check_bwd(c, dx, dw, f"{name} pair tile {tile} splits {sd}/{sw}")


@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("name", ["odd5x5", "pm4x4", "corner16", "s1_1x1"])
def test_pair_modes_exact(native_ext, name, mode):
    """conv_pair_mode 0 (two launches) and 3 (the shipped policy) with automatic tiles / splits."""
    from ddp_amd.ops.layers import conv_backward
    c = _case(SHAPES[name])
    dw = _dw_start(c)
    native_ext.conv_pair_mode(mode)
    try:
        dx = conv_backward(c["spec"], c["xn"], c["dzn"], dw, True)
        torch.cuda.synchronize()
    finally:
        native_ext.conv_pair_mode(3)
    _check_bwd(c, dx, dw, f"{name} pair mode {mode}")


@pytest.mark.parametrize("dense", [1, 0])
@pytest.mark.parametrize("N", [5, 32])
def test_dense2x2_forward_and_pair_exact(native_ext, N, dense):
    """2x2 images: the dense form (one GEMM over whole images) and the implicit GEMM it replaces,
    forward through the layer entry point and backward as the pair."""
    from ddp_amd.ops.layers import conv_backward, conv_forward
    shape = (N, 64, 2, 2, 64, 3, 1, 1)
    c = _case(shape)
    assert native_ext.conv_dense2x2_ok(c["spec"].geom(N, 2, 2))
    dw = _dw_start(c)
    stats = torch.zeros(16 * 2 * 64, device=DEV)
    native_ext.conv_dense2x2_set(dense)
    try:
        z = conv_forward(c["spec"], c["xn"], c["conv"].bias, stats)
        dx = conv_backward(c["spec"], c["xn"], c["dzn"], dw, True)
        torch.cuda.synchronize()
    finally:
        native_ext.conv_dense2x2_set(1)
    _check_fwd(c, z, stats, 64, f"2x2 N={N} dense={dense}")
    _check_bwd(c, dx, dw, f"2x2 N={N} dense={dense}")


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("staged", [0, 1])
@pytest.mark.parametrize("tile", [0, 4])
def test_dgrad_accumulating_and_deferred_exact(native_ext, tile, staged, splits):
    """dx += dgrad onto integers, and dx = dgrad + (mask bit ? acc_dy : 0) onto a deferred first
    branch, for a 1x1 convolution: direct stores, LDS-staged rows and the split-K finish."""
    from ddp_amd.ops.common import ptr, stream_handle, workspace
    from ddp_amd.ops.layers import _masked
    shape = (4, 64, 14, 14, 256, 1, 1, 0)
    N, C, H, W, K = shape[:5]
    c = _case(shape)
    spec = c["spec"]
    ws, s = workspace(torch.device(DEV)), stream_handle()
    g = spec.geom(N, H, W)
    acc = int_tensor((N, H, W, C), -3, 3, 91).to(BF16).to(DEV)
    g_ = torch.Generator().manual_seed(92)
    mask = torch.randint(0, 256, (N, H, W, C // 8), generator=g_, dtype=torch.uint8).to(DEV)
    stored = _masked(acc, mask)
    bits = ((mask.unsqueeze(-1).long() >> torch.arange(8, device=DEV)) & 1).reshape(acc.shape)
    assert torch.equal(stored.float(), acc.float() * bits)
    native_ext.conv_force_tile(tile, 0)
    native_ext.conv_epi_stage_set(staged)
    try:
        dxa = stored.clone()
        native_ext.conv_dgrad(g, ptr(c["dzn"]), ptr(spec.wc), ptr(dxa), ptr(ws), ws.numel(),
                              splits, s, accumulate=1)
        dxd = torch.full_like(c["xn"], float("nan"))
        native_ext.conv_dgrad(g, ptr(c["dzn"]), ptr(spec.wc), ptr(dxd), ptr(ws), ws.numel(),
                              splits, s, accumulate=1, acc_dy=ptr(acc), acc_mask=ptr(mask))
        torch.cuda.synchronize()
    finally:
        native_ext.conv_force_tile(0, 0)
        native_ext.conv_epi_stage_set(1)
    st = stored.double().cpu()
    for name, got in (("accumulate", dxa), ("deferred", dxd)):
        assert_exact(got, c["ref"]["dx"] + st, c["mag"]["dx"] + st.abs(), NHWC, name + " dx")


@pytest.mark.parametrize("fmt", [torch.contiguous_format, torch.channels_last])
def test_wgrad_padded_layer0_exact(native_ext, fmt):
    """The input layer (3 real channels in 8): its weight gradient has only the real channels,
    and nothing before or behind it may be written (the five padded channels have no element)."""
    from ddp_amd.ops.layers import conv_backward
    shape = (2, 8, 32, 32, 64, 3, 1, 1)
    c = _case(shape, creal=3)
    n = 64 * 3 * 3 * 3
    guard = 256
    buf = torch.full((n + 2 * guard,), 12345.0, device=DEV)
    dw = buf[guard:guard + n].view(64, 3, 3, 3)
    if fmt == torch.channels_last:
        dw = buf[guard:guard + n].view(64, 3, 3, 3).permute(0, 3, 1, 2)  # [K][R][S][C] memory
    assert dw.is_contiguous(memory_format=fmt)
    dw.copy_(c["dw0"])
    conv_backward(c["spec"], c["xn"], c["dzn"], dw, False)
    torch.cuda.synchronize()
    _check_bwd(c, None, dw, "layer 0")
    assert bool((buf[:guard] == 12345.0).all()) and bool((buf[guard + n:] == 12345.0).all())


# ------------------------------------------------------------------ conv_tr.hip
@pytest.mark.parametrize("case", TR_CASES)
def test_tap_reuse_forward_exact(native_ext, case):
    from ddp_amd.ops.common import ptr, stream_handle, workspace
    nat = native_ext
    N, C, H, K, BM, BN, splits, stages = case
    c = _case((N, C, H, H, K, 3, 1, 1), bwd=False)
    spec = c["spec"]
    ws, s = workspace(torch.device(DEV)), stream_handle()
    z = torch.full((N, H, H, K), float("nan"), device=DEV, dtype=BF16)
    stats = torch.zeros(16 * 2 * K, device=DEV)
    nat.conv_tr_set(3, 0, 0, 0, 0, BM, BN, splits, stages)
    try:
        r = nat.conv_fwd_tr(spec.geom(N, H, H), ptr(c["xn"]), ptr(spec.wc), ptr(c["conv"].bias),
                            ptr(z), ptr(stats), ptr(ws), ws.numel(), s)
    finally:
        nat.conv_tr_set(3, 0, 0, 0, 0, 0, 0, 0, 0)
    torch.cuda.synchronize()
    assert r == 1, "the forced tap-reuse configuration must be served"
    _check_fwd(c, z, stats, K, f"tap reuse {case}")


@pytest.mark.parametrize("case", TR_DECLINE_CASES)
def test_tap_reuse_small_images_exact(native_ext, case):
    """W = 4 / 8 with batches that do or do not fill whole tiles: served exactly, or declined
    with nothing written."""
    from ddp_amd.ops.common import ptr, stream_handle, workspace
    nat = native_ext
    N, C, H, K, BM, BN, splits = case
    c = _case((N, C, H, H, K, 3, 1, 1), bwd=False)
    spec = c["spec"]
    ws, s = workspace(torch.device(DEV)), stream_handle()
    z = torch.full((N, H, H, K), float("nan"), device=DEV, dtype=BF16)
    stats = torch.zeros(16 * 2 * K, device=DEV)
    nat.conv_tr_set(3, 0, 0, 0, 0, BM, BN, splits, 0)
    try:
        r = nat.conv_fwd_tr(spec.geom(N, H, H), ptr(c["xn"]), ptr(spec.wc), ptr(c["conv"].bias),
                            ptr(z), ptr(stats), ptr(ws), ws.numel(), s)
    finally:
        nat.conv_tr_set(3, 0, 0, 0, 0, 0, 0, 0, 0)
    torch.cuda.synchronize()
    whole = N % (BM // (H * H)) == 0
    assert bool(r) == whole
    if whole:
        _check_fwd(c, z, stats, K, f"tap reuse {case}")
    else:
        assert torch.isnan(z.float()).all() and float(stats.abs().sum()) == 0.0


# ------------------------------------------------------------------ conv_smallk.hip / conv_l0.hip
@pytest.mark.parametrize("shape", [(2, 8, 32, 32, 64, 7, 2, 3), (3, 8, 40, 40, 64, 7, 2, 3),
                                   (2, 8, 32, 32, 64, 3, 1, 1)])
def test_smallk_forward_exact(native_ext, shape):
    """The direct MFMA kernel of the C = 8 input layers: the two 7x7 stem cases (the second with a
    partial last pixel-tile group) and the 3x3 VGG input layer."""
    from ddp_amd.ops.common import ptr, stream_handle
    N, C, H, W, K = shape[:5]
    c = _case(shape, creal=3, bwd=False)
    spec = c["spec"]
    z = torch.full((N, c["P"], c["Q"], K), float("nan"), device=DEV, dtype=BF16)
    stats = torch.zeros(16 * 2 * K, device=DEV)
    served = native_ext.conv_fwd_smallk(spec.geom(N, H, W), ptr(c["xn"]), ptr(spec.wc),
                                        ptr(c["conv"].bias), ptr(z), ptr(stats), stream_handle())
    torch.cuda.synchronize()
    assert served
    _check_fwd(c, z, stats, K, f"smallk {shape}")


def test_l0_statistics_pass_exact(native_ext):
    """conv_l0.hip recomputes z; its statistics pass must give the integer sums of z and z^2."""
    from ddp_amd.ops.common import ptr, stream_handle
    nat = native_ext
    N, K, H = 4, 64, 32
    c = _case((N, 8, H, H, K, 3, 1, 1), creal=3)
    spec = c["spec"]
    g = spec.geom(N, H, H)
    assert nat.l0_ok(g)
    gamma, beta = torch.ones(K, device=DEV), torch.zeros(K, device=DEV)
    stats = torch.zeros(16 * 2 * K, device=DEV)
    coef = torch.full((6 * K,), float("nan"), device=DEV)
    y = torch.full((N, H // 2, H // 2, K), float("nan"), device=DEV, dtype=BF16)
    code = torch.full((N, H // 2, H // 2, K), 0xEE, device=DEV, dtype=torch.uint8)
    zw = torch.full((N, H // 2, H // 2, K), float("nan"), device=DEV, dtype=BF16)
    nat.l0_fwd(g, ptr(c["xn"]), ptr(spec.wc), ptr(c["conv"].bias), 1e-5, 1, ptr(stats), ptr(gamma),
               ptr(beta), ptr(coef), ptr(y), ptr(code), ptr(zw), stream_handle())
    torch.cuda.synchronize()
    _check_stats(c, stats, K, "l0")


# ------------------------------------------------------------------ classifier head (linear_ce.hip)
HEAD_SHAPES = [(B, Fi, J) for B in (1, 3, 64, 67) for Fi in (8, 72, 512, 1024) for J in (1, 10, 16)]


def _head_case(B, Fi, J):
    key = ("head", B, Fi, J)
    if key not in _CACHE:
        x = int_tensor((B, Fi), -2, 2, 31)
        W = int_tensor((J, Fi), -2, 2, 32)
        b = int_tensor((J,), -3, 3, 33)
        dl = int_tensor((B, J), -2, 2, 34)
        dW0, db0 = int_tensor((J, Fi), -5, 5, 35), int_tensor((J,), -5, 5, 36)
        xd, Wd, dld = x.double(), W.double(), dl.double()
        _CACHE[key] = dict(
            x=x.to(BF16).to(DEV), W=W.to(DEV), b=b.to(DEV), dl=dl.to(DEV), dW0=dW0, db0=db0,
            logits=xd @ Wd.t() + b.double(), alogits=xd.abs() @ Wd.abs().t() + b.abs().double(),
            dx=dld @ Wd, adx=dld.abs() @ Wd.abs(), dW=dld.t() @ xd, adW=dld.abs().t() @ xd.abs(),
            db=dld.sum(0), adb=dld.abs().sum(0))
    return _CACHE[key]


@pytest.mark.parametrize("B,Fi,J", HEAD_SHAPES)
def test_linear_ce_fwd_logits_exact(native_ext, B, Fi, J):
    """B not a multiple of the 4 rows of a block, F not a multiple of 64 or of the 512 features a
    wave walks per pass, J = 1 and J = kMaxJ."""
    from ddp_amd.ops.common import ptr, stream_handle
    c = _head_case(B, Fi, J)
    logits = torch.full((B, J), float("nan"), device=DEV)
    native_ext.linear_ce_fwd(ptr(c["x"]), ptr(c["W"]), ptr(c["b"]), 0, B, Fi, J, ptr(logits), 0, 0,
                             0, stream_handle())
    torch.cuda.synchronize()
    assert_exact(logits, c["logits"], c["alogits"], ("b", "j"), "logits")


@pytest.mark.parametrize("gscale", [None, 4.0])
@pytest.mark.parametrize("B,Fi,J", HEAD_SHAPES)
def test_linear_bwd_exact(native_ext, B, Fi, J, gscale):
    """dx = g dl W (bf16), dW += g dl^T x and db += g sum_b dl onto integers (fp32, float atomics
    over 8-row chunks); g = 1 as a null pointer, g = 4 as a device scalar."""
    from ddp_amd.ops.common import ptr, stream_handle
    c = _head_case(B, Fi, J)
    g = 1.0 if gscale is None else gscale
    gs = None if gscale is None else torch.tensor([gscale], device=DEV)
    dx = torch.full((B, Fi), float("nan"), device=DEV, dtype=BF16)
    dW, db = c["dW0"].to(DEV), c["db0"].to(DEV)
    native_ext.linear_bwd(ptr(c["dl"]), ptr(c["x"]), ptr(c["W"]), B, Fi, J, ptr(gs), ptr(dx),
                          ptr(dW), ptr(db), stream_handle())
    torch.cuda.synchronize()
    assert_exact(dx, g * c["dx"], g * c["adx"], ("b", "f"), "dx")
    assert_exact(dW, c["dW0"].double() + g * c["dW"], c["dW0"].abs().double() + g * c["adW"],
                 ("j", "f"), "dW")
    assert_exact(db, c["db0"].double() + g * c["db"], c["db0"].abs().double() + g * c["adb"],
                 ("j",), "db")


@pytest.mark.parametrize("B,Fi,J", [(3, 72, 17), (3, 12, 10)])
def test_head_refuses_bad_shapes(native_ext, B, Fi, J):
    """J above kMaxJ or F not a multiple of 8: the error code, and nothing written."""
    from ddp_amd.ops.common import ptr, stream_handle
    x = torch.ones(B, Fi, device=DEV, dtype=BF16)
    W, b = torch.ones(J, Fi, device=DEV), torch.ones(J, device=DEV)
    y = torch.zeros(B, dtype=torch.int64, device=DEV)
    dl_in = torch.ones(B, J, device=DEV)
    outs = [torch.full((B, J), float("nan"), device=DEV) for _ in range(2)]
    loss = torch.full((1,), float("nan"), device=DEV)
    dx = torch.full((B, Fi), float("nan"), device=DEV, dtype=BF16)
    dW, db = torch.full((J, Fi), float("nan"), device=DEV), torch.full((J,), float("nan"), device=DEV)
    s = stream_handle()
    with pytest.raises(RuntimeError, match="invalid arguments"):
        native_ext.linear_ce_fwd(ptr(x), ptr(W), ptr(b), ptr(y), B, Fi, J, ptr(outs[0]),
                                 ptr(outs[1]), ptr(loss), 0, s)
    with pytest.raises(RuntimeError, match="invalid arguments"):
        native_ext.linear_bwd(ptr(dl_in), ptr(x), ptr(W), B, Fi, J, 0, ptr(dx), ptr(dW), ptr(db), s)
    torch.cuda.synchronize()
    for t in outs + [loss, dx, dW, db]:
        assert bool(torch.isnan(t.float()).all())


# ------------------------------------------------------------------ pool.hip
@pytest.mark.parametrize("B,J", [(37, 10), (64, 17), (256, 1000)])
def test_colsum_exact(native_ext, B, J):
    from ddp_amd.ops.common import ptr, stream_handle
    dl = int_tensor((B, J), -3, 3, 41)
    db0 = int_tensor((J,), -5, 5, 42)
    db = db0.to(DEV)
    native_ext.colsum(ptr(dl.to(BF16).to(DEV)), B, J, ptr(db), stream_handle())
    torch.cuda.synchronize()
    assert_exact(db, db0.double() + dl.double().sum(0), db0.abs().double() + dl.abs().double().sum(0),
                 ("j",), "db")


@pytest.mark.parametrize("N,C,H", [(3, 24, 2), (8, 64, 4), (5, 2048, 8)])
def test_global_avg_pool_power_of_two_exact(native_ext, N, C, H):
    """A power-of-two pixel count: the integer sum times 2**-k is exact, one bf16 rounding."""
    from ddp_amd.ops.common import ptr, stream_handle
    x = int_tensor((N, H, H, C), -3, 3, 51)
    y = torch.full((N, C), float("nan"), device=DEV, dtype=BF16)
    native_ext.avgpool_fwd(ptr(x.to(BF16).to(DEV)), N, H * H, C, ptr(y), stream_handle())
    torch.cuda.synchronize()
    assert_exact(y, x.double().mean((1, 2)), x.abs().double().sum((1, 2)), ("n", "c"), "mean",
                 unit=1.0 / (H * H))


@pytest.mark.parametrize("N,C", [(8, 2048), (3, 24)])
def test_global_avg_pool_7x7_bound(native_ext, N, C):
    """49 pixels: 1 / 49 is not a power of two, so bound mode.

    | rounding                                   | count | pool.hip                          |
    |--------------------------------------------|-------|-----------------------------------|
    | fp32 additions of the 49 terms (any order) | 49    | avgpool_fwd_kernel acc / red sums |
    | inv = 1 / 49 in fp32                       | 1     | ``const float inv``               |
    | sum * inv                                  | 1     | the store expression              |
    | bf16 store                                 | 1     | f2bf                              |

    bound = 2**-8 |ref| + 51 * 2**-24 * T, T = sum |x| / 49 (with integer x the 49 additions are
    in fact exact; the count is kept for any data)."""
    from ddp_amd.ops.common import ptr, stream_handle
    x = int_tensor((N, 7, 7, C), -3, 3, 52)
    y = torch.full((N, C), float("nan"), device=DEV, dtype=BF16)
    native_ext.avgpool_fwd(ptr(x.to(BF16).to(DEV)), N, 49, C, ptr(y), stream_handle())
    torch.cuda.synchronize()
    ref = x.double().mean((1, 2))
    T = x.abs().double().sum((1, 2)) / 49
    e = 51 * FP32_EPS * T
    assert_within(y, ref, BF16_EPS * ref.abs() + (1 + BF16_EPS) * e, ("n", "c"), what="mean 7x7")


# ------------------------------------------------------------------ max-pool ties
def _tie_share(x, k, stride, pad):
    """Share of windows of NCHW ``x`` whose maximum occurs more than once."""
    y = F.max_pool2d(x, k, stride, pad)
    u = F.unfold(F.pad(x, (pad,) * 4, value=float("-inf")), k, stride=stride)
    u = u.reshape(x.shape[0], x.shape[1], k * k, -1)
    return float(((u == y.reshape(x.shape[0], x.shape[1], 1, -1)).sum(2) > 1).double().mean())


@pytest.mark.parametrize("N,C,H", [(4, 64, 15), (3, 24, 5)])
def test_maxpool_ties_exact(native_ext, N, C, H):
    """MaxPool2d(3, 2, 1) on integers in {-2..2}: value, and the gradient of every window at the
    one position PyTorch picks (first maximum in row-major window order)."""
    from ddp_amd.ops.common import ptr, stream_handle
    x = int_tensor((N, C, H, H), -2, 2, 61).double()
    assert _tie_share(x, 3, 2, 1) > 0.4, "the inputs must tie in a large share of the windows"
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 3, 2, 1)
    Ho = yr.shape[-1]
    dy = int_tensor((N, C, Ho, Ho), 1, 3, 62).double()
    yr.backward(dy)
    xn, dyn = _to_dev_nhwc(x), _to_dev_nhwc(dy)
    y = torch.full((N, Ho, Ho, C), float("nan"), device=DEV, dtype=BF16)
    idx = torch.full((N, Ho, Ho, C), 0xEE, device=DEV, dtype=torch.uint8)
    dx = torch.full((N, H, H, C), float("nan"), device=DEV, dtype=BF16)
    s = stream_handle()
    native_ext.maxpool_fwd(ptr(xn), N, H, H, C, 3, 3, 2, 1, Ho, Ho, ptr(y), ptr(idx), s)
    native_ext.maxpool_bwd(ptr(dyn), ptr(idx), N, H, H, C, 3, 3, 2, 1, Ho, Ho, ptr(dx), s)
    torch.cuda.synchronize()
    assert int(idx.max()) < 9
    assert_exact(y, _nhwc(yr.detach()), _nhwc(yr.detach().abs()), NHWC, "pooled")
    # positive gradients: dx equals the reference only if every window routed to one position,
    # the reference's (4 windows of at most 3 meet in a pixel: sums stay below 256, exact in bf16)
    assert_exact(dx, _nhwc(xr.grad), _nhwc(xr.grad.abs()), NHWC, "dx")
    assert float(dx.double().sum()) == float(dy.sum())


def _bn_int_setup(N, C, H, relu, seed):
    """Integer z and BatchNorm inputs that keep y = gamma * z + beta integral: statistics with
    sum z = 0 and sum z^2 = M / 2, eps = 0.5, so mean = 0, var + eps = 1 and invstd = rsqrt(1) =
    1 exactly; gamma = +-1, integer beta. (The statistics are an input of the kernels, so they
    need not be those of z.)"""
    z = int_tensor((N, C, H, H), -2, 2, seed).double()
    gamma = (int_tensor((C,), 0, 1, seed + 1) * 2 - 1)
    beta = int_tensor((C,), -1, 1, seed + 2)
    M = N * H * H
    stats = torch.zeros(16, 2 * C)
    stats[3, C:] = M / 2
    zr = z.clone().requires_grad_(True)
    y = zr * gamma.double().view(1, C, 1, 1) + beta.double().view(1, C, 1, 1)
    y.retain_grad()
    a = F.relu(y) if relu else y
    return z, zr, y, a, gamma, beta, stats


def _bn_bwd_ref(z, dyb, gamma, M):
    """dz = sc (dy_bn - k1 - xhat k2) with xhat = z, sc = gamma, k1 = S1 / M, k2 = S2 / M, and
    the bound of the kernel's fp32 evaluation (bn_act.hip):

    | rounding                              | count | where                                     |
    |---------------------------------------|-------|-------------------------------------------|
    | S1, S2: integer sums                  | 0     | reduce kernels / atomics (exact)          |
    | inv_m = 1 / M, S * inv_m              | 2     | bn_finalize_bwd_kernel, FOLD, local (k1)  |
    | the same for k2                       | 2     |                                           |
    | xhat * k2, two subtractions           | 3     | apply: sc * (dyb - k1 - xh * k2)          |
    | sc * (...) with sc = +-1              | 0     |                                           |
    | bf16 store of dz                      | 1 bf16| f2bf                                      |
    """
    C = z.shape[1]
    s1 = dyb.sum((0, 2, 3))
    s2 = (dyb * z).sum((0, 2, 3))
    k1, k2 = (s1 / M).view(1, C, 1, 1), (s2 / M).view(1, C, 1, 1)
    gm = gamma.double().view(1, C, 1, 1)
    dz = gm * (dyb - k1 - z * k2)
    T = dyb.abs() + k1.abs() + (z * k2).abs()
    e = 7 * FP32_EPS * T
    return dz, BF16_EPS * dz.abs() + (1 + BF16_EPS) * e, s1, s2


@pytest.mark.parametrize("local", [0, 64])
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("N,C,H", [(4, 64, 8), (3, 24, 6)])
def test_bn_act_pool2_ties(native_ext, N, C, H, relu, local):
    """The 2x2 pool inside bn_act_fwd / bn_act_bwd on integral BatchNorm outputs (negative gamma
    on about half of the channels, so pooling before or after the affine map differ): the pooled
    value is exact; dgamma = sum dy_bn * z and dbeta = sum dy_bn are exact integers, which pins
    the routing; dz is checked per element in bound mode with the routing of F.max_pool2d."""
    from ddp_amd.ops.common import ptr, stream_handle
    nat = native_ext
    z, zr, y, a, gamma, beta, stats = _bn_int_setup(N, C, H, relu, 71)
    assert _tie_share(a.detach(), 2, 2, 0) > 0.3
    out_ref = F.max_pool2d(a, 2, 2)
    dout = int_tensor((N, C, H // 2, H // 2), 1, 3, 74).double()
    out_ref.backward(dout)
    dyb = y.grad  # the gradient at the BN output: pool routing and ReLU mask of the reference
    dz_ref, dz_bound, s1, s2 = _bn_bwd_ref(z, dyb, gamma, N * H * H)
    zn, doutn = _to_dev_nhwc(z), _to_dev_nhwc(dout)
    gd, bd, sd = gamma.to(DEV), beta.to(DEV), stats.to(DEV)
    out = torch.full((N, H // 2, H // 2, C), float("nan"), device=DEV, dtype=BF16)
    coef = torch.full((6 * C,), float("nan"), device=DEV)
    s = stream_handle()
    sums = torch.zeros(16 * 2 * C, device=DEV)
    dz = torch.full((N, H, H, C), float("nan"), device=DEV, dtype=BF16)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    nat.bn_act_fwd(N, H, H, C, 1, relu, 0.5, ptr(zn), 0, ptr(sd), ptr(gd), ptr(bd), ptr(out), s,
                   coef=ptr(coef))
    torch.cuda.synchronize()
    cf = coef.view(6, C).cpu()
    assert torch.equal(cf[0], gamma) and torch.equal(cf[1], beta), "scale / shift not integral"
    assert float(cf[2].abs().max()) == 0.0 and bool((cf[3] == 1.0).all())
    o = out_ref.detach()
    assert_exact(out, _nhwc(o), _nhwc(o.abs()), NHWC, "pooled y")
    refused = local == 0 and 256 % (C // 8) != 0  # 3 channel groups do not tile the reduce chain
    nat.bn_bwd_local_set(local)
    try:
        assert bool(nat.bn_bwd_local_ok(N, H, H, C, 1)) == (local != 0)
        if refused:
            with pytest.raises(RuntimeError, match="invalid arguments"):
                nat.bn_act_bwd(N, H, H, C, 1, relu, 0.5, ptr(zn), 0, ptr(sd), ptr(gd), ptr(bd),
                               ptr(doutn), ptr(sums), ptr(dz), 0, ptr(dg), ptr(db), 0, s, ptr(coef))
        else:
            nat.bn_act_bwd(N, H, H, C, 1, relu, 0.5, ptr(zn), 0, ptr(sd), ptr(gd), ptr(bd),
                           ptr(doutn), ptr(sums), ptr(dz), 0, ptr(dg), ptr(db), 0, s, ptr(coef))
        torch.cuda.synchronize()
    finally:
        nat.bn_bwd_local_set(8)
    if refused:
        assert bool(torch.isnan(dz.float()).all()) and float(dg.abs().sum()) == 0.0
        return
    assert_exact(db, s1, dyb.abs().sum((0, 2, 3)), ("c",), "dbeta")
    assert_exact(dg, s2, (dyb * z).abs().sum((0, 2, 3)), ("c",), "dgamma")
    assert_within(dz, _nhwc(dz_ref.detach()), _nhwc(dz_bound.detach()), NHWC, what="dz")


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("N,C,H", [(4, 64, 15), (3, 32, 5)])
def test_bn_pool3_ties(native_ext, N, C, H, relu):
    """The ResNet stem's BN + ReLU + MaxPool2d(3, 2, 1) pair on integral BatchNorm outputs: pooled
    value exact, dgamma / dbeta exact integers, dz per element with F.max_pool2d's routing.
    (bn_pool3 needs 64 % (C / 8) == 0, so the small case has 32 channels.)"""
    from ddp_amd.ops.common import ptr, stream_handle
    nat = native_ext
    z, zr, y, a, gamma, beta, stats = _bn_int_setup(N, C, H, relu, 81)
    assert _tie_share(a.detach(), 3, 2, 1) > 0.4
    out_ref = F.max_pool2d(a, 3, 2, 1)
    Ho = out_ref.shape[-1]
    dout = int_tensor((N, C, Ho, Ho), 1, 3, 84).double()
    out_ref.backward(dout)
    dyb = y.grad
    dz_ref, dz_bound, s1, s2 = _bn_bwd_ref(z, dyb, gamma, N * H * H)
    zn, doutn = _to_dev_nhwc(z), _to_dev_nhwc(dout)
    gd, bd, sd = gamma.to(DEV), beta.to(DEV), stats.to(DEV)
    out = torch.full((N, Ho, Ho, C), float("nan"), device=DEV, dtype=BF16)
    idx = torch.full((N, Ho, Ho, C), 0xEE, device=DEV, dtype=torch.uint8)
    coef = torch.full((6 * C,), float("nan"), device=DEV)
    sums = torch.zeros(16 * 2 * C, device=DEV)
    dz = torch.full((N, H, H, C), float("nan"), device=DEV, dtype=BF16)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    s = stream_handle()
    nat.bn_pool3_fwd(N, H, H, C, relu, 0.5, ptr(zn), ptr(sd), ptr(gd), ptr(bd), ptr(out), ptr(idx),
                     s, 0, 0, 0.1, 0, ptr(coef))
    nat.bn_pool3_bwd(N, H, H, C, relu, 0.5, ptr(zn), ptr(doutn), ptr(idx), ptr(sums), ptr(dz),
                     ptr(dg), ptr(db), s, ptr(coef))
    torch.cuda.synchronize()
    cf = coef.view(6, C).cpu()
    assert torch.equal(cf[0], gamma) and torch.equal(cf[1], beta), "scale / shift not integral"
    o = out_ref.detach()
    assert_exact(out, _nhwc(o), _nhwc(o.abs()), NHWC, "pooled y")
    assert_exact(db, s1, dyb.abs().sum((0, 2, 3)), ("c",), "dbeta")
    assert_exact(dg, s2, (dyb * z).abs().sum((0, 2, 3)), ("c",), "dgamma")
    assert_within(dz, _nhwc(dz_ref.detach()), _nhwc(dz_bound.detach()), NHWC, what="dz")
