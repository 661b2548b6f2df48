"""Index paths of the conv GEMM kernels (csrc/kernels/conv_igemm.hip, conv_tr.hip) against fp32
PyTorch on the smallest shapes that take each of them.

The per-item index math divides by launch constants through host-precomputed multipliers
(common.h FastDiv): tiles per split, column tiles, images, channels, taps, image rows. These
shapes make every one of those divisors a non-power-of-two somewhere, leave partial row and
column tiles, and walk the pixel-major, dense 2x2, strided-phase and tap-reuse forms with forced
tiles and split counts 1-3. Reference op: torch.nn.functional.conv2d in fp32 and its autograd
backward. Tolerances are those of tests/test_gpu_kernels.py::test_conv_every_tile
and test_conv_bwd_pair_forced_splits (relative l2 error < 1e-2: bf16 operands and outputs,
fp32 accumulation).

The norm alone passes over a local defect (one tile row, one tap of a corner pixel: see
tests/test_exactness_cpu.py), so every comparison is also made per element against an fp64
reference (tests/exactness.py assert_within) with the bound of an fp32-accumulated reduction of n
terms stored with at most one bf16 rounding: 2**-8 |ref| + n * 2**-24 * sum |a b|, where n is
the reduction length -- R*S*C + 1 (bias) for FWD z, K*R*S for DGRAD dx (both bf16), N*P*Q for
WGRAD dw (fp32: no bf16 term). Where the output is bf16 the fp32 term carries the factor
(1 + 2**-8) (exactness.dot_bound): the bf16 rounding acts on the value the kernel computed, not
on the reference, so it is at most 2**-8 (|ref| + fp32 error) -- 0.4 % more on the small term than
the formula above. tests/test_gpu_exact.py runs the same shapes on integers, bitwise.
"""
import pytest
import torch
import torch.nn.functional as F

from exactness import assert_within, dot_bound
from test_gpu_kernels import DEV, _conv_setup, bf, rel_err

pytestmark = pytest.mark.gpu

# name -> N, C, H, W, K, R, stride, pad
SHAPES = {
    "odd5x5": (3, 8, 5, 5, 24, 3, 1, 1),      # M = 75, K = 24: partial tiles, no power of two
    "pm4x4_n3": (3, 64, 4, 4, 64, 3, 1, 1),   # pixel-major switches on / off, N below a tile
    "pm4x4": (64, 64, 4, 4, 64, 3, 1, 1),     # ... and N = one 64-image block: pixel-major runs
    "corner16": (2, 64, 16, 16, 64, 3, 1, 1),  # split 3 of a corner pixel's 4 valid taps is empty
    "corner16_n64": (64, 64, 16, 16, 64, 3, 1, 1),  # ... with pixel-major rows (any image size)
    "dense2x2": (5, 64, 2, 2, 64, 3, 1, 1),   # one dense GEMM per direction, N = 5
    "s2_3x3": (2, 16, 6, 6, 32, 3, 2, 1),     # strided: DGRAD as four phase GEMMs
    "s2_1x1": (2, 16, 6, 6, 32, 1, 2, 0),     # ... and the 1x1 whose odd phases are empty
    "s1_1x1": (2, 16, 6, 6, 32, 1, 1, 0),
}
_CACHE = {}


def _ref64(x, w, b, dz, stride, pad):
    """fp64 z, dx (NHWC) and dw of NCHW operands, and the same on the operands' magnitudes, as
    (reference, bound) pairs for assert_within."""
    def ops(x, w, b, dz):
        xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        F.conv2d(xr, wr, None, stride, pad).backward(dz)
        z = F.conv2d(x, w, b, stride, pad).permute(0, 2, 3, 1).contiguous()
        return z, xr.grad.permute(0, 2, 3, 1).contiguous(), wr.grad
    x, w, b, dz = (t.detach().double().cpu() for t in (x, w, b, dz))
    ref, mag = ops(x, w, b, dz), ops(x.abs(), w.abs(), b.abs(), dz.abs())
    K, C, R, S = w.shape
    n = (R * S * C + 1, K * R * S, dz.shape[0] * dz.shape[2] * dz.shape[3])
    return {k: (ref[i], dot_bound(ref[i], mag[i], n[i], 0 if k == "wgrad" else 1))
            for i, k in enumerate(("fwd", "dgrad", "wgrad"))}


def _elem_bad(bad, key, got, e64, names):
    """The per-element check beside a rel_err: a failure is recorded in ``bad`` like the norm's."""
    try:
        worst = assert_within(got, e64[key][0], e64[key][1], names, what=key)
        print(key, "worst |err| / bound", worst)
    except AssertionError as e:
        bad[key + " per element"] = str(e)


NHWC, KCRS = ("n", "h", "w", "c"), ("k", "c", "r", "s")


def _case(name):
    """Operands and fp32 references of a shape, computed once and shared (never modified)."""
    if name not in _CACHE:
        N, C, H, W, K, R, stride, pad = SHAPES[name]
        torch.manual_seed(1234)
        conv, spec, x, xn = _conv_setup(N, C, H, W, K, R, stride, pad)
        P = (H + 2 * pad - R) // stride + 1
        Q = (W + 2 * pad - R) // stride + 1
        dz = bf(torch.randn(N, K, P, Q, device=DEV))
        dzn = dz.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
        ref = F.conv2d(x, conv.weight, conv.bias, stride, pad).permute(0, 2, 3, 1).contiguous()
        xr = x.clone().requires_grad_(True)
        wr = conv.weight.detach().clone().requires_grad_(True)
        F.conv2d(xr, wr, None, stride, pad).backward(dz)
        _CACHE[name] = dict(conv=conv, spec=spec, x=x, xn=xn, dz=dz, dzn=dzn, ref=ref,
                            dx=xr.grad.permute(0, 2, 3, 1).contiguous(), dw=wr.grad,
                            e64=_ref64(x, conv.weight, conv.bias, dz, stride, pad))
    return _CACHE[name]


def _stats_ok(stats, z, K):
    st = stats.view(16, 2 * K).sum(0)
    zf = z.float().reshape(-1, K)
    return (torch.allclose(st[:K], zf.sum(0), rtol=1e-3, atol=1e-2)
            and torch.allclose(st[K:], (zf * zf).sum(0), rtol=1e-3, atol=1e-2))


def _separate(nat, name, splits, rows_pm=None, wgrad_pm=None):
    """FWD, DGRAD and WGRAD as three launches with a forced split count -> error dict"""
    from ddp_amd.ops.common import ptr, stream_handle, weight_krsc, workspace
    c = _case(name)
    N, C, H, W, K, R, stride, pad = SHAPES[name]
    spec, conv = c["spec"], c["conv"]
    ws, s = workspace(torch.device(DEV)), stream_handle()
    dw = torch.zeros_like(conv.weight, memory_format=torch.channels_last)
    g = spec.geom(N, H, W, weight_krsc(dw))
    z = torch.full_like(c["ref"], float("nan"), dtype=torch.bfloat16)
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
    errs = {"fwd": rel_err(z, c["ref"]), "dgrad": rel_err(dx, c["dx"]), "wgrad": rel_err(dw, c["dw"])}
    print(name, splits, errs)
    bad = {k: v for k, v in errs.items() if not v < 1e-2}
    _elem_bad(bad, "fwd", z, c["e64"], NHWC)
    _elem_bad(bad, "dgrad", dx, c["e64"], NHWC)
    _elem_bad(bad, "wgrad", dw, c["e64"], KCRS)
    if not _stats_ok(stats, z, K):
        bad["stats"] = "BatchNorm statistics of z"
    return bad


@pytest.mark.parametrize("splits", [1, 2, 3])
@pytest.mark.parametrize("tile", range(8))
@pytest.mark.parametrize("name", ["odd5x5", "pm4x4_n3", "corner16", "dense2x2", "s2_3x3", "s2_1x1",
                                  "s1_1x1"])
def test_every_tile_and_split(native_ext, name, tile, splits):
    """FWD, DGRAD and WGRAD on every forced implicit-GEMM tile with 1-3 splits. A forced tile the
    problem cannot run must fall back to one it can: WGRAD's 256-column tiles, and for the dense
    2x2 form every column tile wider than one pixel's 64 channels (conv_igemm.hip tile_ok; before
    that check a forced 128- or 256-column tile computed a wrong forward here)."""
    native_ext.conv_force_tile(tile + 1, 0)
    try:
        bad = _separate(native_ext, name, splits)
    finally:
        native_ext.conv_force_tile(0, 0)
    assert not bad, f"{name} tile {tile} splits {splits}: {bad}"


@pytest.mark.parametrize("splits", [1, 2, 3])
@pytest.mark.parametrize("rows_pm,wgrad_pm", [(0, 0), (1, 1), (2, 2)])
@pytest.mark.parametrize("name", ["pm4x4_n3", "pm4x4", "corner16", "corner16_n64"])
def test_pixel_major_on_and_off(native_ext, name, rows_pm, wgrad_pm, splits):
    """Pixel-major rows (FWD / DGRAD) and reduction (WGRAD) switched off, on for small images and
    on for every image size, on the 64x64 tile a 64-image block fills: with 3 splits the third
    split of a corner pixel (4 valid taps x 1 channel block, 2 k-steps per split) is empty and
    must still write its zero slab."""
    native_ext.conv_force_tile(4, 0)  # 64x64
    try:
        bad = _separate(native_ext, name, splits, rows_pm, wgrad_pm)
    finally:
        native_ext.conv_force_tile(0, 0)
    assert not bad, f"{name} pm {rows_pm}/{wgrad_pm} splits {splits}: {bad}"


@pytest.mark.parametrize("sd,sw", [(1, 1), (2, 3), (3, 2), (3, 3)])
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("name", ["odd5x5", "pm4x4_n3", "pm4x4", "corner16", "dense2x2", "s1_1x1"])
def test_pair_every_tile_and_split(native_ext, name, tile, sd, sw):
    """The backward pair (DGRAD + WGRAD in one launch) on every forced pair tile with DGRAD /
    WGRAD split counts 1-3."""
    from ddp_amd.ops.layers import conv_backward
    c = _case(name)
    dw = torch.zeros_like(c["conv"].weight, memory_format=torch.channels_last)
    native_ext.conv_pair_force(sd, sw, tile)
    try:
        dx = conv_backward(c["spec"], c["xn"], c["dzn"], dw, True)
        torch.cuda.synchronize()
    finally:
        native_ext.conv_pair_force(0, 0, 0)
    errs = {"dgrad": rel_err(dx, c["dx"]), "wgrad": rel_err(dw, c["dw"])}
    print(name, tile, sd, sw, errs)
    bad = {k: v for k, v in errs.items() if not v < 1e-2}
    _elem_bad(bad, "dgrad", dx, c["e64"], NHWC)
    _elem_bad(bad, "wgrad", dw, c["e64"], KCRS)
    assert not bad, f"{name} pair tile {tile} splits {sd}/{sw}: {bad}"


@pytest.mark.parametrize("dense", [1, 0])
def test_dense2x2_forward_and_pair(native_ext, dense):
    """N = 5 images of 2x2: the dense form (one GEMM over whole images) and the implicit GEMM it
    replaces, forward through the layer entry point and backward as the pair."""
    from ddp_amd.ops.layers import conv_backward, conv_forward
    c = _case("dense2x2")
    N, C, H, W, K = SHAPES["dense2x2"][:5]
    assert native_ext.conv_dense2x2_ok(c["spec"].geom(N, H, W))
    dw = torch.zeros_like(c["conv"].weight, memory_format=torch.channels_last)
    stats = torch.zeros(16 * 2 * K, device=DEV)
    native_ext.conv_dense2x2_set(dense)
    try:
        z = conv_forward(c["spec"], c["xn"], c["conv"].bias, stats)
        dx = conv_backward(c["spec"], c["xn"], c["dzn"], dw, True)
        torch.cuda.synchronize()
    finally:
        native_ext.conv_dense2x2_set(1)
    errs = {"fwd": rel_err(z, c["ref"]), "dgrad": rel_err(dx, c["dx"]), "wgrad": rel_err(dw, c["dw"])}
    print(dense, errs)
    assert not {k: v for k, v in errs.items() if not v < 1e-2}, errs
    bad = {}
    _elem_bad(bad, "fwd", z, c["e64"], NHWC)
    _elem_bad(bad, "dgrad", dx, c["e64"], NHWC)
    _elem_bad(bad, "wgrad", dw, c["e64"], KCRS)
    assert not bad, bad
    assert _stats_ok(stats, z, K)


# N, C, H (= W), K, BM, BN, splits: tiles of BM / (H*H) images; N = 6 and N = 3 are not multiples
TR_CASES = [(6, 64, 4, 64, 64, 64, 1), (8, 64, 4, 64, 64, 64, 1), (12, 128, 4, 64, 64, 64, 2),
            (3, 64, 8, 64, 128, 64, 1), (4, 64, 8, 64, 128, 64, 1), (3, 128, 8, 128, 64, 64, 2)]


@pytest.mark.parametrize("fused_in", [False, True])
@pytest.mark.parametrize("case", TR_CASES)
def test_tap_reuse_forward(native_ext, case, fused_in):
    """The tap-reuse forward at W = 4 and W = 8 with a plain input and with the BatchNorm + ReLU
    input computed while the patch loads, z and its statistics against fp32. A tile holds
    BM / (H*W) whole images; when N is no multiple of that the kernel must decline (return 0,
    nothing written) rather than run a tile past the batch, and the implicit GEMM serves it."""
    from ddp_amd.ops.common import ptr, stream_handle, workspace
    nat = native_ext
    N, C, H, K, BM, BN, splits = case
    torch.manual_seed(99)
    conv, spec, x, xn = _conv_setup(N, C, H, H, K, 3, 1, 1)
    ws, s = workspace(torch.device(DEV)), stream_handle()
    g = spec.geom(N, H, H)
    fin = None
    if fused_in:  # x = relu(bn(zin)) of a preceding block with batch statistics
        zin = (torch.randn(N, H, H, C, device=DEV) * 2 + 0.5).to(torch.bfloat16)
        st_in = torch.zeros(16, 2, C, device=DEV)
        zf = zin.float().reshape(-1, C)
        st_in[5, 0] = zf.sum(0)
        st_in[5, 1] = (zf * zf).sum(0)
        gamma = torch.rand(C, device=DEV) + 0.5
        beta = torch.randn(C, device=DEV) * 0.1
        xn = torch.empty(N, H, H, C, device=DEV, dtype=torch.bfloat16)
        nat.bn_act_fwd(N, H, H, C, 0, 1, 1e-5, ptr(zin), 0, ptr(st_in), ptr(gamma), ptr(beta),
                       ptr(xn), s, coef=ptr(torch.zeros(6 * C, device=DEV)))
        x = xn.float().permute(0, 3, 1, 2)
        coef = torch.zeros(6 * C, device=DEV)
        y = torch.full_like(xn, float("nan"))
        fin = (ptr(zin), ptr(st_in), ptr(gamma), ptr(beta), 1e-5, 1, 0, ptr(coef), ptr(y))
    z = torch.full((N, H, H, K), float("nan"), device=DEV, dtype=torch.bfloat16)
    stats = torch.zeros(16 * 2 * K, device=DEV)
    nat.conv_tr_set(3, 0, 0, 0, 0, BM, BN, splits, 0)
    try:
        r = nat.conv_fwd_tr(g, 0 if fused_in else ptr(xn), ptr(spec.wc), ptr(conv.bias), ptr(z),
                            ptr(stats), ptr(ws), ws.numel(), s, None, fin)
    finally:
        nat.conv_tr_set(3, 0, 0, 0, 0, 0, 0, 0, 0)
    torch.cuda.synchronize()
    whole = N % (BM // (H * H)) == 0
    assert bool(r) == whole, "served exactly when the tiles hold whole images of the batch"
    if not whole:
        assert torch.isnan(z.float()).all() and float(stats.abs().sum()) == 0.0
        nat.conv_fwd(g, ptr(xn), ptr(spec.wc), ptr(conv.bias), ptr(z), ptr(stats), ptr(ws),
                     ws.numel(), 0, s)
        torch.cuda.synchronize()
    elif fused_in:
        assert torch.equal(y, xn), "the materialised input equals the separate BatchNorm pass"
    ref = F.conv2d(x, conv.weight, conv.bias, 1, 1).permute(0, 2, 3, 1)
    err = rel_err(z, ref)
    print(case, fused_in, r, err)
    assert err < 1e-2
    bad = {}
    _elem_bad(bad, "fwd", z, _ref64(x, conv.weight, conv.bias, torch.zeros_like(ref).permute(
        0, 3, 1, 2), 1, 1), NHWC)
    assert not bad, bad
    assert _stats_ok(stats, z, K)
