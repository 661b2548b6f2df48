"""Exact-mode tests of the grouped 3x3 kernels (csrc/kernels/conv_group.hip; tests/exactness.py).

Operands as tests/test_gpu_exact.py draws them: x, w in {-1..1}, bias in {-3..3}, dz in {-2..2},
dw0 in {-5..5}. Reductions are at most 9 * 32 terms for z and dx and N * P * Q terms of magnitude
<= 2 for dW, far inside 2**24, so fp32 accumulation is exact in any order. z and dx are stored as
bf16: the set-up checks on the CPU that the reference of every case stays within 256, where bf16
holds every integer. The fp64 reference is F.conv2d(groups=G) and its autograd on the CPU,
computed once per case; outputs are pre-filled with NaN.
"""
import pytest
import torch
import torch.nn.functional as F

from exactness import assert_exact, int_tensor

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
NHWC = ("n", "h", "w", "c")
# N, H, W, C: an odd image below any pixel tile with two slabs; H != W with a partial last tile;
# every tap but the centre is padding; four slabs, WGRAD's pixel split, layer1's width
GEOMS = {"5x5": (2, 5, 5, 64), "9x7": (3, 9, 7, 64), "1x1": (1, 1, 1, 32), "8x8": (2, 8, 8, 128)}
_CACHE = {}


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _ref(x, w, b, dz, stride, G):
    x, w = x.double().requires_grad_(True), w.double().requires_grad_(True)
    z = F.conv2d(x, w, b.double(), stride, 1, groups=G)
    z.backward(dz.double())
    zn = _nhwc(z.detach())
    flat = zn.reshape(-1, zn.shape[-1])
    return dict(z=zn, dx=_nhwc(x.grad), dw=w.grad, s1=flat.sum(0), s2=(flat * flat).sum(0),
                a1=flat.abs().sum(0))


def _case(geom, Cg, stride, seed=11):
    key = (geom, Cg, stride)
    if key not in _CACHE:
        from ddp_amd.ops.layers import ConvBNActSpec
        N, H, W, C = GEOMS[geom]
        P, Q = (H - 1) // stride + 1, (W - 1) // stride + 1
        x = int_tensor((N, C, H, W), -1, 1, seed)
        w = int_tensor((C, Cg, 3, 3), -1, 1, seed + 1)
        b = int_tensor((C,), -3, 3, seed + 2)
        dz = int_tensor((N, C, P, Q), -2, 2, seed + 3)
        ref = _ref(x, w, b, dz, stride, C // Cg)
        assert float(ref["z"].abs().max()) <= 256 and float(ref["dx"].abs().max()) <= 256, \
            "choose another seed: a bf16 output of this case is not an exact integer"
        conv = torch.nn.Conv2d(C, C, 3, stride, 1, groups=C // Cg, bias=True).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(w)
            conv.bias.copy_(b)
        spec = ConvBNActSpec(conv, None)
        spec.maybe_pack()
        _CACHE[key] = dict(conv=conv, spec=spec, xn=_nhwc(x).to(BF16).to(DEV),
                           dzn=_nhwc(dz).to(BF16).to(DEV), ref=ref,
                           mag=_ref(x.abs(), w.abs(), b.abs(), dz.abs(), stride, C // Cg),
                           dw0=int_tensor((C, Cg, 3, 3), -5, 5, seed + 4))
    return _CACHE[key]


def _run_and_check(c, what):
    from ddp_amd.ops.common import stat_replicas
    from ddp_amd.ops.layers import conv_backward, conv_forward
    spec, ref, mag = c["spec"], c["ref"], c["mag"]
    K = spec.K
    stats = torch.zeros(stat_replicas() * 2 * K, device=DEV)
    z = conv_forward(spec, c["xn"], c["conv"].bias, stats)
    assert_exact(z, ref["z"], mag["z"], NHWC, what + " z")
    st = stats.view(-1, 2 * K).sum(0).cpu()
    assert_exact(st[:K], ref["s1"], ref["a1"], ("k",), what + " sum z")
    assert_exact(st[K:], ref["s2"], ref["s2"], ("k",), what + " sum z^2")
    for fmt in (torch.contiguous_format, torch.channels_last):  # [K][Cg][3][3] and [K][3][3][Cg]
        dw = c["dw0"].to(DEV).contiguous(memory_format=fmt)
        dx = conv_backward(spec, c["xn"], c["dzn"], dw, True)
        assert_exact(dx, ref["dx"], mag["dx"], NHWC, what + " dx")
        assert_exact(dw, ref["dw"] + c["dw0"].double(), mag["dw"] + c["dw0"].abs().double(),
                     ("k", "c", "r", "s"), what + f" dw0 + dW ({fmt})")


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("Cg", [4, 8, 16, 32])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_grouped_conv_exact(native_ext, geom, Cg, stride):
    """z, the summed statistics replicas, dx and dw0 + dW in both master layouts, per element."""
    _run_and_check(_case(geom, Cg, stride), f"{geom} Cg={Cg} stride {stride}")


def test_pad_channels_of_cg4_do_not_contribute(native_ext):
    """Cg = 4: the operand copy's four pad channels hold a non-zero pattern."""
    c = _case("5x5", 4, 1)
    wc = c["spec"].wc
    assert wc.shape[-1] == 8
    keep = wc.clone()
    try:
        wc[..., 4:] = torch.arange(1, 5, device=DEV, dtype=BF16)
        _run_and_check(c, "pad channels set")
    finally:
        wc.copy_(keep)


@pytest.mark.parametrize("what,C,K,groups,R", [("Cg = 2", 64, 64, 32, 3), ("C != K", 64, 128, 4, 3),
                                               ("C = 48", 48, 48, 6, 3), ("R = 1", 64, 64, 8, 1)])
def test_geometries_outside_the_range_are_refused(native_ext, what, C, K, groups, R):
    g = (2, 8, 8, C, K, R, R, 1, R // 2, 8, 8, C // groups, 0)
    assert not native_ext.gconv_ok(g, groups), what
    assert native_ext.gconv_ok((2, 8, 8, 64, 64, 3, 3, 1, 1, 8, 8, 8, 0), 8)
