"""Per-element tests of the soft-target loss kernels (linear_ce.hip, the SOFT instantiations) and
of the mixed batch kernel (data.hip augment_kernel<MIX>), bound mode of tests/exactness.py.

The bounds extend ``ce_bounds`` of tests/test_gpu_elementwise.py (whose terms for exp, log, the
sums and the stores are kept as they are) by the soft target, counted from linear_ce.hip SoftRow:

| quantity                                          | roundings                                  |
|---------------------------------------------------|--------------------------------------------|
| t_j = fma(1 - E, wa [j=ya] + wb [j=yb], E / J)    | 1 - E, wb = 1 - lam, E / J, the fma: 4, each|
|                                                   | of a quantity <= t_j: 4 u t_j              |
| s = fma(E/J, sum_j z_j, (1-E) fma(wa,z_ya,wb z_yb))| the sum of J logits (J - 1), wb z_yb, two  |
|                                                   | fma, one product: at most J + 4, each of a |
|                                                   | quantity <= sum_j |t_j z_j|; plus the error|
|                                                   | of t: sum_j 4 u t_j |z_j|                  |
| d_j = (p_j - t_j) * inv_b                         | dp_j + dt_j, then 3 as in ce_bounds        |
| loss = sum_b (lse - s) * inv_b                    | as in ce_bounds with s for l_y             |

E and lam are the fp32 values the kernels receive. No element is excluded: the soft loss has no
branch that the reference cannot decide.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from exactness import BF16_EPS as b_, FP32_EPS as u_, assert_within, mismatches
from test_gpu_elementwise import (EPS, ROW_KINDS, _ce_row, _dev_nhwc, _head_inputs, _logit_terms,
                                  _rexp, bn_fwd_terms)

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
E_LAM = [(0.1, 1.0), (0.0, 0.3), (0.1, 0.3), (0.1, 0.0)]


def f32(v):
    return float(np.float32(v))


def soft_ce_bounds(logits, ya, yb, E, lam, dl_in, n_sum, out_bf16):
    """fp64 soft-target mean cross-entropy of [B][J] ``logits`` (known to the kernel within
    ``dl_in``), dlogits = (softmax - t) / B, and their bounds (module docstring; the softmax
    part is ce_bounds line for line)."""
    B, J = logits.shape
    E, lam = f32(E), f32(lam)
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
    t = (1 - E) * (lam * F.one_hot(ya, J).double() + (1 - lam) * F.one_hot(yb, J).double()) + E / J
    dt = 4 * u_ * t
    d = (p - t) / B
    dd = (dp + dt) / B + 3 * u_ * d.abs()
    d_bound = b_ * d.abs() + (1 + b_) * dd if out_bf16 else dd
    tz = (t * logits).abs().sum(1, keepdim=True)
    s = (t * logits).sum(1, keepdim=True)
    ds = (dt * logits.abs() + t * dl_in).sum(1, keepdim=True) + (J + 4) * u_ * tz
    terms = (lse - s) / B
    loss = terms.sum()
    loss_bound = ((dlse + ds + u_ * (lse - s).abs()) / B + 2 * u_ * terms.abs()).sum() \
        + B * u_ * terms.abs().sum()
    return loss, loss_bound, d, d_bound


def torch_soft_loss(logits, ya, yb, E, lam):
    """The issue's definition through torch: lam CE(ya) + (1 - lam) CE(yb), label_smoothing=E."""
    E, lam = f32(E), f32(lam)
    return lam * F.cross_entropy(logits, ya, label_smoothing=E) \
        + (1 - lam) * F.cross_entropy(logits, yb, label_smoothing=E)


def _partner(labels, J, other):
    """yb per row: equal to ya on the rows where ``other`` is False, a different class else."""
    yb = labels.clone()
    for i in range(len(labels)):
        if other[i] and J > 1:
            yb[i] = (int(labels[i]) + 1 + i) % J
            if yb[i] == labels[i]:
                yb[i] = (int(labels[i]) + 1) % J
    return yb


# ------------------------------------------------------------------ softmax_ce, soft
@pytest.mark.parametrize("E,lam", E_LAM)
@pytest.mark.parametrize("out_bf16", [0, 1])
@pytest.mark.parametrize("in_bf16", [0, 1])
@pytest.mark.parametrize("J", [1, 10, 257, 1000])
@pytest.mark.parametrize("B", [1, 5])
def test_softmax_ce_soft_per_element(native_ext, B, J, in_bf16, out_bf16, E, lam):
    """Loss, correct and every dlogits element of softmax_ce(soft=...), the row kinds of
    test_softmax_ce_per_element, each with yb == ya and with yb != ya."""
    from ddp_amd.ops.common import ptr, stream_handle
    batches = [ROW_KINDS] if B == 5 else [[k] for k in ROW_KINDS]
    lam_d = torch.tensor([lam], dtype=torch.float32, device=DEV)
    for kinds in batches:
        rows = [_ce_row(k, J, 400 + J + i) for i, k in enumerate(kinds)]
        logits = torch.stack([r for r, _ in rows])
        ya = torch.tensor([l for _, l in rows], dtype=torch.int64)
        for start in (0, 1):  # which rows get a partner of another class
            yb = _partner(ya, J, [(i + start) % 2 == 1 for i in range(B)])
            ld = logits.to(BF16 if in_bf16 else torch.float32).to(DEV)
            loss = torch.zeros((), device=DEV)
            correct = torch.zeros((), dtype=torch.int32, device=DEV)
            dl = torch.full((B, J), float("nan"), device=DEV,
                            dtype=BF16 if out_bf16 else torch.float32)
            ybd = yb.to(DEV)
            native_ext.softmax_ce(ptr(ld), in_bf16, ptr(ya.to(DEV)), B, J, ptr(loss),
                                  ptr(correct), ptr(dl), out_bf16, stream_handle(),
                                  soft=(E, ptr(ybd), ptr(lam_d)))
            torch.cuda.synchronize()
            want, loss_bound, d, d_bound = soft_ce_bounds(logits, ya, yb, E, lam,
                                                          torch.zeros_like(logits), J, out_bf16)
            assert torch.allclose(want, torch_soft_loss(logits, ya, yb, E, lam),
                                  rtol=1e-11, atol=1e-11)
            first = torch.tensor([int(torch.nonzero(r == r.max())[0]) for r in logits])
            assert int(correct) == int((first == ya).sum()), kinds  # argmax == ya, as plain
            what = f"{kinds} partner rows {start}"
            print("loss", assert_within(loss.cpu().double().view(1), want.view(1),
                                        loss_bound.view(1), what="loss " + what))
            print("dlogits", assert_within(dl, d, d_bound, ("b", "j"), what="dlogits " + what))
            assert_within(dl.double().sum(1).cpu(), torch.zeros(B, dtype=torch.float64),
                          d_bound.sum(1), ("b",), what="row sums " + what)


def test_softmax_ce_soft_refuses_bad_smoothing(native_ext):
    from ddp_amd.ops.common import ptr, stream_handle
    ld = torch.zeros(2, 10, device=DEV)
    y = torch.zeros(2, dtype=torch.int64, device=DEV)
    dl = torch.full((2, 10), float("nan"), device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    for e in (1.0, -0.1):
        with pytest.raises(RuntimeError, match="invalid arguments"):
            native_ext.softmax_ce(ptr(ld), 0, ptr(y), 2, 10, ptr(loss), 0, ptr(dl), 0,
                                  stream_handle(), soft=(e, 0, 0))
    torch.cuda.synchronize()
    assert bool(torch.isnan(dl).all()) and bool(torch.isnan(loss).all())


# ------------------------------------------------------------------ fused head, soft
def _head_setup(B, Fi, J, seed):
    z, gamma, beta, W, bias, labels = _head_inputs(B, Fi, J, seed)
    t = bn_fwd_terms(z, gamma, beta)
    dev = dict(zn=_dev_nhwc(z), g=gamma.to(DEV), b=beta.to(DEV), st=t["stats"].to(DEV),
               W=W.to(DEV), bias=bias.to(DEV), y=labels.to(DEV))
    return W, bias, labels, dev


def _run_head(nat, dv, B, Fi, J, fused, soft=None, x_in=None):
    """One head launch into NaN-filled outputs: (features, coef, dlogits, loss)."""
    from ddp_amd.ops.common import ptr, stream_handle
    kw = {"soft": soft} if soft is not None else {}
    dl = torch.full((B, J), float("nan"), device=DEV)
    loss = torch.zeros((), device=DEV)
    if fused:
        x = torch.full((B, Fi), float("nan"), device=DEV, dtype=BF16)
        coef = torch.full((6 * Fi,), float("nan"), device=DEV)
        nat.bn_pool_linear_ce_fwd(ptr(dv["zn"]), ptr(dv["st"]), ptr(dv["g"]), ptr(dv["b"]), EPS, 1,
                                  ptr(coef), ptr(x), ptr(dv["W"]), ptr(dv["bias"]), ptr(dv["y"]),
                                  B, Fi, J, ptr(dl), ptr(loss), stream_handle(), **kw)
    else:
        x, coef = x_in, None
        nat.linear_ce_fwd(ptr(x), ptr(dv["W"]), ptr(dv["bias"]), ptr(dv["y"]), B, Fi, J, 0,
                          ptr(dl), ptr(loss), 0, stream_handle(), **kw)
    torch.cuda.synchronize()
    return x, coef, dl, loss


@pytest.mark.parametrize("E,lam", E_LAM)
@pytest.mark.parametrize("Fi", [64, 1024])
@pytest.mark.parametrize("B", [3, 6])
def test_fused_head_soft(native_ext, B, Fi, E, lam):
    """linear_ce_fwd and bn_pool_linear_ce_fwd with soft targets: loss and dlogits per element
    against fp64 on the stored bf16 features; the features and the coefficient table bit-equal
    to the plain call's. Partner labels = the labels reversed (rows with yb != ya, and with
    B = 3 the middle row with yb == ya). B = 6: a full block and a half-empty one."""
    from ddp_amd.ops.common import ptr
    J = 10
    W, bias, labels, dv = _head_setup(B, Fi, J, 500 + Fi)
    yb = labels.flip(0).contiguous()
    ybd = yb.to(DEV)
    lam_d = torch.tensor([lam], dtype=torch.float32, device=DEV)
    soft = (E, ptr(ybd), ptr(lam_d))
    x0, coef0, _, _ = _run_head(native_ext, dv, B, Fi, J, True)
    x1, coef1, dl_f, loss_f = _run_head(native_ext, dv, B, Fi, J, True, soft)
    assert torch.equal(x1.view(torch.int16), x0.view(torch.int16)), "features"
    assert torch.equal(coef1[:4 * Fi].view(torch.int32), coef0[:4 * Fi].view(torch.int32)), "coef"
    assert bool(torch.isnan(coef1[4 * Fi:]).all())
    _, _, dl_s, loss_s = _run_head(native_ext, dv, B, Fi, J, False, soft, x_in=x0)
    logits, dlog = _logit_terms(x0.double().cpu(), W, bias)
    want, loss_bound, d, d_bound = soft_ce_bounds(logits, labels, yb, E, lam, dlog, J, 0)
    assert torch.allclose(want, torch_soft_loss(logits, labels, yb, E, lam), rtol=1e-11, atol=1e-11)
    for name, got_l, got_d in (("fused", loss_f, dl_f), ("separate", loss_s, dl_s)):
        print(name, "loss", assert_within(got_l.cpu().double().view(1), want.view(1),
                                          loss_bound.view(1), what=name + " loss"))
        print(name, "dlogits", assert_within(got_d, d, d_bound, ("b", "j"),
                                             what=name + " dlogits"))
        assert_within(got_d.double().sum(1).cpu(), torch.zeros(B, dtype=torch.float64),
                      d_bound.sum(1), ("b",), what=name + " row sums")


# ------------------------------------------------------------------ neutral element, bitwise
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("B", [3, 6])
def test_head_soft_neutral_is_plain(native_ext, B, fused):
    """E = 0, lam = 1, yb = ya through the soft instantiations: dlogits torch.equal to the plain
    call's; the loss too at B = 3 (one block, one atomic add)."""
    from ddp_amd.ops.common import ptr
    J, Fi = 10, 64
    _, _, _, dv = _head_setup(B, Fi, J, 700)
    one = torch.ones(1, device=DEV)
    x0, _, dl0, loss0 = _run_head(native_ext, dv, B, Fi, J, True)
    if not fused:
        _, _, dl0, loss0 = _run_head(native_ext, dv, B, Fi, J, False, x_in=x0)
    for soft in ((0.0, ptr(dv["y"]), ptr(one)), (0.0, 0, 0), (0.0, ptr(dv["y"]), 0)):
        _, _, dl1, loss1 = _run_head(native_ext, dv, B, Fi, J, fused, soft, x_in=x0)
        assert torch.equal(dl1, dl0), soft
        if B == 3:
            assert torch.equal(loss1, loss0), soft


@pytest.mark.parametrize("J", [10, 257, 1000])
@pytest.mark.parametrize("bf16", [0, 1])
def test_softmax_ce_soft_neutral_is_plain(native_ext, J, bf16):
    from ddp_amd.ops.common import ptr, stream_handle
    one = torch.ones(1, device=DEV)
    for B in (1, 5):
        kinds = ROW_KINDS[:B]
        rows = [_ce_row(k, J, 800 + J + i) for i, k in enumerate(kinds)]
        ld = torch.stack([r for r, _ in rows]).to(BF16 if bf16 else torch.float32).to(DEV)
        y = torch.tensor([l for _, l in rows], dtype=torch.int64, device=DEV)
        out = []
        for kw in ({}, {"soft": (0.0, ptr(y), ptr(one))}, {"soft": (0.0, 0, 0)}):
            loss = torch.zeros((), device=DEV)
            dl = torch.full((B, J), float("nan"), device=DEV, dtype=ld.dtype)
            native_ext.softmax_ce(ptr(ld), bf16, ptr(y), B, J, ptr(loss), 0, ptr(dl), bf16,
                                  stream_handle(), **kw)
            torch.cuda.synchronize()
            out.append((dl, loss))
        for dl, loss in out[1:]:
            assert not bool(mismatches(dl.cpu(), out[0][0].cpu()).any())
            if B == 1:
                assert torch.equal(loss, out[0][1])


# ------------------------------------------------------------------ the mixed batch kernel
GUARD = 64
PAT = {torch.bfloat16: (torch.int16, 0x7fc5), torch.float32: (torch.int32, 0x7fc12345),
       torch.int64: (torch.int64, 0x5a5a5a5a5a5a5a5a)}


class Buf:
    """n elements between two guard bands of a non-canonical pattern; compared whole, as bits."""

    def __init__(self, n, dtype):
        self.bits, pat = PAT[dtype]
        self.n = n
        self.full = torch.full((n + 2 * GUARD,), pat, dtype=self.bits, device=DEV)
        self.inner = self.full[GUARD:GUARD + n].view(dtype)

    def assert_is(self, inner, what):
        want = torch.full_like(self.full, PAT[inner.dtype][1]).cpu()
        want[GUARD:GUARD + self.n] = inner.contiguous().cpu().reshape(-1).view(self.bits)
        got = self.full.cpu()
        bad = torch.nonzero(got != want).reshape(-1)
        assert bad.numel() == 0, (f"{what}: {bad.numel()} elements differ bitwise, first at "
                                  f"{[i - GUARD for i in bad[:8].tolist()]} (guards < 0 or >= n)")


H = W = 32
CP = 8
LAMS = [0.25, 1.0, 0.0, 0.8125 + 2.0 ** -20]


@pytest.fixture(scope="module")
def mix_data():
    """A 23-sample dataset, a 7-sample shard order and the fp64 augmented pixels of every
    sample, computed once."""
    from ddp_amd.data import SyntheticCIFAR10, CIFAR_MEAN, CIFAR_STD
    from ddp_amd.data.loader import crop_flip_params
    ds = SyntheticCIFAR10(True, n=23)
    imgs, labels = ds.cpu_arrays()
    order = np.array([5, 22, 0, 17, 9, 3, 11], dtype=np.int32)
    epoch = 3
    cy, cx, fl = crop_flip_params(ds.seed, epoch, np.arange(23), 4, True)
    mean = np.asarray(CIFAR_MEAN, np.float32).astype(np.float64)
    inv = (np.float32(1) / np.asarray(CIFAR_STD, np.float32)).astype(np.float64)
    aug, mag = np.zeros((23, H, W, 3)), np.zeros((23, H, W, 3))
    for i in range(23):
        padded = np.zeros((H + 8, W + 8, 3))
        padded[4:4 + H, 4:4 + W] = imgs[i]
        crop = padded[cy[i]:cy[i] + H, cx[i]:cx[i] + W]
        crop = crop[:, ::-1] if fl[i] else crop
        aug[i] = (crop / 255.0 - mean) * inv
        mag[i] = (crop / 255.0 + mean) * inv  # the same expression on its terms' magnitudes
    dimg, dlab = ds.device_arrays(torch.device(DEV))
    return dict(ds=ds, imgs=imgs, labels=labels, order=order, epoch=epoch,
                aug=torch.from_numpy(aug), mag=torch.from_numpy(mag), dimg=dimg, dlab=dlab,
                didx=torch.from_numpy(order).to(DEV))


def _augment(nat, md, B, cursor, off, mix=None):
    from ddp_amd.data import CIFAR_MEAN, CIFAR_STD
    from ddp_amd.ops.common import ptr, stream_handle
    x, y = Buf(B * H * W * CP, BF16), Buf(B, torch.int64)
    cur = torch.tensor([cursor], dtype=torch.int32, device=DEV)
    kw = {"cursor_off": off} if off else {}
    y2 = lc = None
    if mix is not None:
        y2, lc = Buf(B, torch.int64), Buf(1, torch.float32)
        kw["mix"] = (y2.inner.data_ptr(), ptr(mix), mix.numel(), lc.inner.data_ptr())
    nat.augment(ptr(md["dimg"]), ptr(md["dlab"]), ptr(md["didx"]), ptr(cur), len(md["order"]), B,
                H, W, CP, 4, 1, md["ds"].seed & 0xFFFFFFFF, md["epoch"], CIFAR_MEAN, CIFAR_STD,
                x.inner.data_ptr(), y.inner.data_ptr(), stream_handle(), **kw)
    torch.cuda.synchronize()
    return x, y, y2, lc


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("cursor", [0, 3])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_augment_mix(native_ext, mix_data, B, cursor, off):
    """augment(mix=...): x per element against fp64 from the uint8 sources within
    2^-8 |ref| (the bf16 store) + 8 * 2^-24 (|a| + |b|), where |a| and |b| are, as everywhere in
    bound mode (tests/exactness.py), the sums of their terms' magnitudes (raw / 255 + mean) *
    inv_std: a = (raw * (1/255) - mean) * inv_std takes 5 fp32 roundings (both constants, two
    products, the difference: a green value of 123 cancels against mean = 123 / 255 down to the
    rounding of its terms), the blend 3 more. y, y2 and lam_cur exact; lam = 1 gives
    the unmixed kernel's batch and lam = 0 that batch reversed, bit for bit; every buffer whole
    with its guard bands. cursor 3 (x B = 5, shard of 7) wraps ``pos`` around the shard."""
    from ddp_amd.data import augment_cpu
    md = mix_data
    L = len(md["order"])
    table = torch.tensor(LAMS, dtype=torch.float32, device=DEV)
    k = (cursor + off) % len(LAMS)
    lam = f32(LAMS[k])
    pos = [((cursor + off) * B + b) % L for b in range(B)]
    idx = md["order"][pos]
    a = md["aug"][idx]                      # [B][H][W][3] fp64
    p = md["aug"][idx[::-1].copy()]
    ref = lam * a + (1 - lam) * p
    rev = idx[::-1].copy()
    bound = b_ * ref.abs() + 8 * u_ * (md["mag"][idx] + md["mag"][rev])
    x, y, y2, lc = _augment(native_ext, md, B, cursor, off, table)
    got = x.inner.view(B, H, W, CP)
    print("x", assert_within(got[..., :3], ref, bound, ("b", "h", "w", "c"), what="mixed x"))
    want_x = got.clone()  # channels 0..2 are within the bound; the pad channels must be 0
    want_x[..., 3:] = 0
    x.assert_is(want_x, "x")
    labels = torch.from_numpy(md["labels"][idx].astype(np.int64))
    y.assert_is(labels, "y")
    y2.assert_is(labels.flip(0), "y2")
    lc.assert_is(torch.tensor([lam], dtype=torch.float32), "lam_cur")
    plain, yp, _, _ = _augment(native_ext, md, B, cursor, off)
    yp.assert_is(labels, "plain y")
    pv = plain.inner.view(B, H, W, CP)
    if lam == 1.0:
        x.assert_is(pv, "lam = 1 is the unmixed batch")
    if lam == 0.0:
        x.assert_is(pv.flip(0), "lam = 0 is the unmixed batch reversed")
    # the numpy twin: one bf16 ulp, the comparison test_gpu_kernels.py makes for the plain batch
    cpu = augment_cpu(md["imgs"], idx, md["ds"].seed, md["epoch"], True, lam=np.float32(lam))
    assert torch.allclose(got[..., :3].permute(0, 3, 1, 2).float().cpu(), cpu, rtol=8e-3, atol=1e-2)


def test_augment_mix_lam_zero(native_ext, mix_data):
    """Table entry 2 (lam = 0): cursor 2."""
    md = mix_data
    table = torch.tensor(LAMS, dtype=torch.float32, device=DEV)
    for B in (1, 2, 5):
        x, _, _, lc = _augment(native_ext, md, B, 2, 0, table)
        plain, _, _, _ = _augment(native_ext, md, B, 2, 0)
        lc.assert_is(torch.zeros(1), "lam_cur")
        x.assert_is(plain.inner.view(B, H, W, CP).flip(0), "lam = 0 is the unmixed batch reversed")


def test_augment_mix_refuses_missing_pointers(native_ext, mix_data):
    from ddp_amd.data import CIFAR_MEAN, CIFAR_STD
    from ddp_amd.ops.common import ptr, stream_handle
    md = mix_data
    x, y = Buf(H * W * CP, BF16), Buf(1, torch.int64)
    t = torch.ones(1, device=DEV)
    for mix in ((0, ptr(t), 1, ptr(t)), (y.inner.data_ptr(), ptr(t), 0, ptr(t)),
                (y.inner.data_ptr(), ptr(t), 1, 0)):
        with pytest.raises(RuntimeError, match="invalid arguments"):
            native_ext.augment(ptr(md["dimg"]), ptr(md["dlab"]), ptr(md["didx"]), 0, 7, 1, H, W,
                               CP, 4, 1, 1, 0, CIFAR_MEAN, CIFAR_STD, x.inner.data_ptr(),
                               y.inner.data_ptr(), stream_handle(), mix=mix)
    torch.cuda.synchronize()
    x.assert_is(x.inner.clone(), "x untouched")
