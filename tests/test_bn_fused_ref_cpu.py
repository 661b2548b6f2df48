"""tests/bn_fused_ref.py proved without a GPU.

* ``bn_bwd_ref`` (autograd routing) against a plain per-window Python loop on a tiny case, and
  against ``bn_bwd_routed`` (the explicit routing) on the shapes the GPU tests use: identical,
  pooled and unpooled, with and without ReLU.
* The inputs do what tests/test_gpu_bn_fused_exact.py relies on: about half of the pool windows
  tie, about a third are cut by the ReLU, every intermediate of dz is an fp32 number where M is a
  power of two (asserted inside ``bn_bwd_ref``).
* Each defect a fused kernel could have changes the reference S1, S2 or dz by a non-zero amount on
  these inputs -- the evidence that the bitwise GPU comparisons would fail on it:
    1. one dgrad row dropped from the sums,
    2. the last maximum of a window instead of the first,
    3. one window's gradient sent to the neighbouring pixel,
    4. M off by the pool factor (inv_m from the dgrad's rows, not z's pixels),
    5. dgamma / dbeta written (=) instead of accumulated (+=),
    6. one 16-channel block skipped (its outputs keep their pre-fill).
* The signed-zero rule of ``assert_dz_exact``: -0 and +0 compare equal, anything else does not.
"""
import pytest
import torch
import torch.nn.functional as F

from bn_fused_ref import (BF16, UNIT, assert_dz_exact, bn_bwd_ref, bn_bwd_routed, coef_table, cv,
                          representable, win, z_tensor)
from exactness import assert_exact, int_tensor

# dgrad geometry (N, C, H, W, K) of the GPU tests' fused-finish shapes, 3x3 / stride 1 / pad 1
SHAPES = [(8, 64, 4, 4, 64), (32, 64, 2, 2, 64), (8, 48, 4, 4, 64), (3, 64, 4, 4, 64),
          (5, 64, 2, 2, 64), (3, 8, 5, 5, 24)]
_DATA = {}


def _data(shape, pool, relu):
    key = (shape, pool, relu)
    if key not in _DATA:
        N, C, H, W, K = shape
        dy = int_tensor((N, K, H, W), -2, 2, 10).double()
        w = int_tensor((K, C, 3, 3), -1, 1, 8).double()
        dx = F.conv_transpose2d(dy, w, None, 1, 1)  # DGRAD of the 3x3 / s1 / p1 convolution
        m = 2 if pool else 1
        z = z_tensor(N, C, m * H, m * W, 21)
        coef = coef_table(C, 22)
        _DATA[key] = (dx, z, coef, bn_bwd_ref(dx, z, coef, pool, relu))
    return _DATA[key]


def _loop_ref(dx, z, coef, pool, relu):
    """The rule of bn_act.hip bwd_compute, one window at a time."""
    N, C, Hz, Wz = z.shape
    sc, sh = coef[0].double(), coef[1].double()
    dxb = dx.to(BF16).double()
    dyb = torch.zeros_like(z)
    for n in range(N):
        for c in range(C):
            for h in range(dxb.shape[2]):
                for w_ in range(dxb.shape[3]):
                    pix = [(2 * h + d // 2, 2 * w_ + d % 2) for d in range(4)] if pool \
                        else [(h, w_)]
                    best, arg = None, None
                    for (i, j) in pix:
                        y = float(z[n, c, i, j] * sc[c] + sh[c])
                        yr = max(y, 0.0) if relu else y
                        if best is None or yr > best:  # strict: the first maximum stays
                            best, arg, yarg = yr, (i, j), y
                    if not relu or yarg > 0:
                        dyb[n, c, arg[0], arg[1]] = dxb[n, c, h, w_]
    return dyb


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("pool", [1, 0])
def test_reference_matches_window_loop(pool, relu):
    shape = (2, 8, 3, 3, 8)
    dx, z, coef, r = _data(shape, pool, relu)
    assert torch.equal(r["dyb"], _loop_ref(dx, z, coef, pool, relu))
    M = z.numel() // z.shape[1]
    mu, is_, sc = (coef[i].double() for i in (2, 3, 0))
    xh = (z - cv(mu)) * cv(is_)
    S1, S2 = r["dyb"].sum((0, 2, 3)), (r["dyb"] * xh).sum((0, 2, 3))
    assert torch.equal(r["S1"], S1) and torch.equal(r["S2"], S2)
    assert torch.equal(r["dz"], cv(sc) * (r["dyb"] - cv(S1 / M) - xh * cv(S2 / M)))


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("pool", [1, 0])
@pytest.mark.parametrize("shape", SHAPES)
def test_autograd_and_explicit_routing_agree(shape, pool, relu):
    dx, z, coef, r = _data(shape, pool, relu)
    q = bn_bwd_routed(dx, z, coef, pool, relu)
    for k in ("dyb", "S1", "S2", "dz"):
        assert torch.equal(r[k], q[k]), k
    assert bool((r["S1"] == r["S1"].round()).all()) and bool((r["S2"] / UNIT == (r["S2"] / UNIT).round()).all())
    assert r["pow2"] == (shape[0] in (8, 32))


def test_inputs_tie_and_cut():
    dx, z, coef, r = _data(SHAPES[0], 1, 1)
    y = z * cv(coef[0].double()) + cv(coef[1].double())
    yw = win(F.relu(y))
    ties = float(((yw == yw.max(-1, keepdim=True).values).sum(-1) > 1).double().mean())
    cut = float((yw.max(-1).values <= 0).double().mean())
    print(f"ties {ties:.2f} relu-cut windows {cut:.2f} max|dx| {float(dx.abs().max()):.0f} "
          f"A1 {float(r['A1'].max()):.0f} A2 {float(r['A2'].max()):.0f}")
    assert ties > 0.4 and 0.2 < cut < 0.5
    assert float(dx.abs().max()) > 64  # the gradients are far from the {-2..2} of the operands
    # non-argmax pixels of a window receive sc * (-k1 - xhat * k2), not 0
    off = (r["dyb"] == 0) & (r["dz"] != 0)
    assert float(off.double().mean()) > 0.3


def _change(r, q):
    return {k: float((r[k] - q[k]).abs().max()) for k in ("S1", "S2", "dz")}


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[3]])
def test_defects_change_the_reference(shape):
    """Defects 1-4 on the pooled, ReLU case (4 also unpooled: M is then right, no change)."""
    N, C, H, W, K = shape
    dx, z, coef, r = _data(shape, 1, 1)
    rows = N * H * W
    found = {}
    found["dropped row"] = _change(r, bn_bwd_routed(dx, z, coef, 1, 1, drop_row=rows - 1))
    found["last maximum"] = _change(r, bn_bwd_routed(dx, z, coef, 1, 1, tie="last"))
    # a window that carries a gradient: the first nonzero routed element's window
    n, c, i, j = torch.nonzero(r["dyb"])[0].tolist()
    found["neighbour pixel"] = _change(r, bn_bwd_routed(dx, z, coef, 1, 1,
                                                        neighbour=(n, c, i // 2, j // 2)))
    found["M off by the pool factor"] = _change(r, bn_bwd_routed(dx, z, coef, 1, 1, m_factor=4))
    for name, d in found.items():
        print(f"{shape} {name}: max change S1 {d['S1']:g} S2 {d['S2']:g} dz {d['dz']:g}")
    assert found["dropped row"]["S1"] > 0 and found["dropped row"]["S2"] > 0
    assert found["last maximum"]["S2"] > 0 and found["last maximum"]["dz"] > 0
    # (S1 does not see the routing inside a window whose pixels are all positive: S2 and dz do)
    assert found["neighbour pixel"]["S2"] > 0 or found["neighbour pixel"]["S1"] > 0
    assert found["neighbour pixel"]["dz"] > 0
    assert found["M off by the pool factor"]["dz"] > 0
    assert found["M off by the pool factor"]["S1"] == 0  # only dz shows a wrong inv_m
    # the changes survive dz's bf16 store
    q = bn_bwd_routed(dx, z, coef, 1, 1, m_factor=4)
    assert not torch.equal(q["dz"].to(BF16), r["dz"].to(BF16))


def test_assignment_instead_of_accumulation_and_skipped_block_show():
    """Defects 5 and 6 against the checks the GPU tests apply to dgamma / dbeta / sums."""
    dx, z, coef, r = _data(SHAPES[0], 1, 1)
    C = z.shape[1]
    pre = int_tensor((C,), -5, 5, 30)
    assert float(pre.abs().min()) == 0 and int((pre != 0).sum()) > C // 2
    want, mag = pre.double() + r["S2"], pre.abs().double() + r["A2"]
    assert_exact((pre.double() + r["S2"]).float(), want, mag, ("c",), "dgamma", unit=UNIT)
    with pytest.raises(AssertionError, match="dgamma"):  # = instead of +=
        assert_exact(r["S2"].float(), want, mag, ("c",), "dgamma", unit=UNIT)
    skipped = (pre.double() + r["S1"]).float()
    skipped[16:32] = pre[16:32]                           # channels 16..31 never added
    print(f"skipped block: max change {float((skipped.double() - pre - r['S1']).abs().max()):g}")
    with pytest.raises(AssertionError, match="dbeta"):
        assert_exact(skipped, pre.double() + r["S1"], pre.abs().double() + r["A1"], ("c",),
                     "dbeta")


def test_dz_comparison_ignores_only_the_sign_of_zero():
    ref = torch.tensor([0.0, -0.0, 1.5, -3.0, 0.0], dtype=torch.float64)
    got = torch.tensor([-0.0, 0.0, 1.5, -3.0, 0.0]).to(BF16)
    assert_dz_exact(got, ref)
    bad = got.clone()
    bad[2] = 1.5078125  # one bf16 ulp
    with pytest.raises(AssertionError, match="1 of 5"):
        assert_dz_exact(bad, ref)
    with pytest.raises(AssertionError, match="1 of 5"):
        assert_dz_exact(torch.tensor([0.0, 0.0, 1.5, -3.0, float("nan")]).to(BF16), ref)
    assert representable(torch.tensor([0.1], dtype=torch.float32).double())
    assert not representable(torch.tensor([0.1], dtype=torch.float64))
