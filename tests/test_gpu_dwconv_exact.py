"""Exact-mode tests of the depthwise 3x3 kernels (csrc/kernels/dwconv.hip; tests/exactness.py).

Operands: x, w in {-1..1}, bias in {-3..3}, dz in {-2..2}, dw0 in {-5..5}. Then |z| <= 9 + 3 = 12
and |dx| <= 9 * 2 = 18, so every bf16 store is an exact integer, and the dW and statistics sums
(at most N * P * Q terms of magnitude <= 2 resp. 144) stay far below 2**24: fp32 accumulation is
exact in any order. The fp64 reference is F.conv2d(groups=C) and its autograd on the CPU, computed
once per case; outputs are pre-filled with NaN.
"""
import pytest
import torch
import torch.nn.functional as F

from exactness import assert_exact, int_tensor

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
NHWC = ("n", "h", "w", "c")
# N, H, W, C
GEOMS = {
    "1x1": (1, 1, 1, 8),       # every tap but the centre is padding; one chunk, 255 idle lanes
    "2x2": (2, 2, 2, 32),      # MobileNet's CIFAR tail: 2x2 -> 1x1 at stride 2
    "5x5": (2, 5, 5, 40),      # odd image; five chunk lanes (not a power of two)
    "9x7": (3, 9, 7, 64),      # H != W; three images share a block's column slots
    # wider than a block's column tile (C = 128: 16 chunk lanes x 16 columns, W = 19 -> two
    # tiles of 10 and 9 columns) and taller than a band (16 rows -> bands of 10 and 9); its 8
    # (stride 2: 2) tiles make the WGRAD plan use that many pixel splits
    "19x19": (2, 19, 19, 128),
    # 8 chunk groups x 260 tiles: above 2048 work items a forward block walks two tiles with its
    # statistics in registers, and WGRAD's 128 splits take two to three tiles each
    "1x9": (260, 1, 9, 1024),
}
_CACHE = {}


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _ref(x, w, b, dz, stride):
    x, w = x.double().requires_grad_(True), w.double().requires_grad_(True)
    z = F.conv2d(x, w, b.double(), stride, 1, groups=x.shape[1])
    z.backward(dz.double())
    zn = _nhwc(z.detach())
    flat = zn.reshape(-1, zn.shape[-1])
    return dict(z=zn, dx=_nhwc(x.grad), dw=w.grad, s1=flat.sum(0), s2=(flat * flat).sum(0),
                a1=flat.abs().sum(0))


def _case(geom, stride, seed=23):
    key = (geom, stride)
    if key not in _CACHE:
        from ddp_amd.ops.layers import ConvBNActSpec
        N, H, W, C = GEOMS[geom]
        P, Q = (H - 1) // stride + 1, (W - 1) // stride + 1
        x = int_tensor((N, C, H, W), -1, 1, seed)
        w = int_tensor((C, 1, 3, 3), -1, 1, seed + 1)
        b = int_tensor((C,), -3, 3, seed + 2)
        dz = int_tensor((N, C, P, Q), -2, 2, seed + 3)
        conv = torch.nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=True).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(w)
            conv.bias.copy_(b)
        spec = ConvBNActSpec(conv, None)
        assert spec.depthwise
        spec.maybe_pack()
        _CACHE[key] = dict(conv=conv, spec=spec, xn=_nhwc(x).to(BF16).to(DEV),
                           dzn=_nhwc(dz).to(BF16).to(DEV), ref=_ref(x, w, b, dz, stride),
                           mag=_ref(x.abs(), w.abs(), b.abs(), dz.abs(), stride),
                           dw0=int_tensor((C, 1, 3, 3), -5, 5, seed + 4))
    return _CACHE[key]


def _run_and_check(c, what):
    from ddp_amd.ops.common import (native, ptr, stat_replicas, stream_handle, weight_krsc,
                                    workspace)
    spec, ref, mag, xn, dzn = c["spec"], c["ref"], c["mag"], c["xn"], c["dzn"]
    K, nan, s = spec.K, float("nan"), stream_handle()
    N, H, W, _ = xn.shape
    stats = torch.zeros(stat_replicas() * 2 * K, device=DEV)
    z = torch.full_like(dzn, nan)
    native().dwconv_fwd(spec.geom(N, H, W), K, ptr(xn), ptr(spec.wc), ptr(c["conv"].bias), ptr(z),
                        ptr(stats), s)
    assert_exact(z, ref["z"], mag["z"], NHWC, what + " z")
    st = stats.view(-1, 2 * K).sum(0).cpu()
    assert_exact(st[:K], ref["s1"], ref["a1"], ("k",), what + " sum z")
    assert_exact(st[K:], ref["s2"], ref["s2"], ("k",), what + " sum z^2")
    ws = workspace(xn.device)
    for fmt in (torch.contiguous_format, torch.channels_last):  # [K][1][3][3] and [K][3][3][1]
        dw = c["dw0"].to(DEV).contiguous(memory_format=fmt)
        g = spec.geom(N, H, W, weight_krsc(dw))
        dx = torch.full_like(xn, nan)
        native().dwconv_wgrad(g, K, ptr(dzn), ptr(xn), ptr(dw), ptr(ws), ws.numel(), s)
        native().dwconv_dgrad(g, K, ptr(dzn), ptr(spec.wc), ptr(dx), s)
        assert_exact(dx, ref["dx"], mag["dx"], NHWC, what + " dx")
        assert_exact(dw, ref["dw"] + c["dw0"].double(), mag["dw"] + c["dw0"].abs().double(),
                     ("k", "c", "r", "s"), what + f" dw0 + dW ({fmt})")


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_depthwise_conv_exact(native_ext, geom, stride):
    """z, the summed statistics replicas, dx and dw0 + dW in both master layouts, per element."""
    _run_and_check(_case(geom, stride), f"{geom} stride {stride}")


def test_pad_elements_of_the_operand_copy_do_not_contribute(native_ext):
    """Elements 1..7 of each 8-element pitch of Wc hold a non-zero pattern."""
    c = _case("5x5", 2)
    wc = c["spec"].wc
    assert wc.shape[-1] == 8
    keep = wc.clone()
    try:
        wc[..., 1:] = torch.arange(1, 8, device=DEV, dtype=BF16)
        _run_and_check(c, "pad elements set")
    finally:
        wc.copy_(keep)


@pytest.mark.parametrize("what,C,K,R,stride,pad", [("5x5", 64, 64, 5, 1, 2), ("K = 2C", 64, 128, 3, 1, 1),
                                                   ("C = 12", 12, 12, 3, 1, 1), ("stride 3", 64, 64, 3, 3, 1),
                                                   ("pad 0", 64, 64, 3, 1, 0)])
def test_geometries_outside_the_range_are_refused(native_ext, what, C, K, R, stride, pad):
    P = (8 + 2 * pad - R) // stride + 1
    assert not native_ext.dwconv_ok((2, 8, 8, C, K, R, R, stride, pad, P, P, 1, 0), C), what
    assert native_ext.dwconv_ok((2, 8, 8, 64, 64, 3, 3, 1, 1, 8, 8, 1, 0), 64)
    if what == "5x5":
        from ddp_amd.ops.layers import ConvBNActSpec
        conv = torch.nn.Conv2d(C, K, R, stride, pad, groups=C, bias=False).cuda()
        with pytest.raises(ValueError, match="channels per group"):
            ConvBNActSpec(conv, torch.nn.BatchNorm2d(K).cuda())
