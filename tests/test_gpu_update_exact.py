"""The kernels that write the model's state -- csrc/kernels/optim.hip -- against the CPU oracle
of tests/update_oracle.py, element for element and bit for bit.

Every device buffer has a guard band of 64 elements on each side filled with a non-canonical
pattern (fp32 0x7fc12345, bf16 0x7fc5, int32 0x5a5a5a5a). WHOLE buffers are compared, as integer
views: the guards and every element that no work item owns must come back unchanged.

Exact mode: lr 2**-2, momentum 2**-1, wd 2**-3, grad_scale 2**-1, p / g / buf integers in
[-64, 64], two steps (fresh integer gradients each). The oracle asserts that every intermediate
is an fp32 number, so no fp32 operation rounds, contracted to fma or not, and p, buf and the bf16
copies (which round for real, ties of both parities included) must equal the oracle.

Bound mode: randn inputs, lr 0.1, momentum 0.9, wd 1e-4, grad_scale 0.5, one step on a non-zero
momentum history. |err| <= R * 2**-24 * T with T the oracle's pass over the magnitudes and R the
roundings counted in common.h sgd_update1:
    g * grad_scale (1), fma(wd, p, .) (2), fma(momentum, buf, .) (3)      -> buf: R = 3
    [nesterov: fma(momentum, buf, d) (4)], fma(-lr, d, p) (4 or 5)         -> p:   R = 4 or 5
Elements the oracle leaves unchanged get bound 0. The bf16 copies are compared bitwise with
bf16(the kernel's own new p).
"""
import numpy as np
import pytest
import torch

import update_oracle as uo
from exactness import FP32_EPS, assert_exact, assert_within, coords, int_tensor, mismatches

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64
EXACT = dict(lr=2.0 ** -2, momentum=2.0 ** -1, wd=2.0 ** -3, grad_scale=2.0 ** -1)
PROJECT = dict(lr=0.1, momentum=0.9, wd=1e-4, grad_scale=0.5)
PATTERN = {torch.float32: (torch.int32, 0x7fc12345), torch.bfloat16: (torch.int16, 0x7fc5),
           torch.int32: (torch.int32, 0x5a5a5a5a), torch.uint8: (torch.uint8, 0xA5)}
R_BUF = 3


def r_p(nesterov):
    return 5 if nesterov else 4


def stream():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """n elements between two guard bands; ``inner`` is a view, ``ptr`` its device address."""

    def __init__(self, n, dtype=torch.float32, fill=None):
        bits, pat = PATTERN[dtype]
        self.n, self.dtype = n, dtype
        self.full = torch.full((n + 2 * GUARD,), pat, dtype=bits, device=DEV).view(dtype)
        self.inner = self.full[GUARD:GUARD + n]
        if fill is not None:
            self.set(fill)

    @property
    def ptr(self):
        return self.inner.data_ptr()

    def set(self, t):
        self.inner.copy_(torch.as_tensor(t).to(self.dtype).reshape(-1))

    def host(self):
        return self.full.cpu()

    def expect(self, before, inner):
        """The whole buffer a correct launch leaves: ``before`` (host image) with ``inner``."""
        w = before.clone()
        w[GUARD:GUARD + self.n] = inner.to(self.dtype).reshape(-1)
        return w

    def np_bits(self):
        return uo.bf16_to_bits(self.inner)


def same_bits(got, want, what, shape=None, names=None, guard=GUARD):
    """Bitwise equality of two host tensors through exactness.mismatches (bf16 / fp32 views of
    the other types); a failure lists the first elements, guards as negative flat indices
    (``guard=0``: the tensors have no guard bands)."""
    got, want = got.cpu().contiguous(), want.cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.dtype == torch.int32:
        got, want = got.view(torch.float32), want.view(torch.float32)
    bad = (got != want) if got.dtype == torch.uint8 else mismatches(got, want)
    bad = bad.reshape(-1)
    if not bool(bad.any()):
        return
    idx = torch.nonzero(bad).reshape(-1)
    bits = {torch.float32: torch.int32, torch.bfloat16: torch.int16}.get(got.dtype, got.dtype)
    lines = []
    for i in idx[:8].tolist():
        j = i - guard
        where = (coords(j, shape) if shape is not None and 0 <= j < int(np.prod(shape)) else j)
        lines.append(f"  {names or 'index'} {where}: got {float(got.reshape(-1)[i])!r} "
                     f"(0x{int(got.reshape(-1).view(bits)[i]) & 0xffffffff:x}) want "
                     f"{float(want.reshape(-1)[i])!r} "
                     f"(0x{int(want.reshape(-1).view(bits)[i]) & 0xffffffff:x})")
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ bitwise; "
                         f"first {len(lines)}:\n" + "\n".join(lines))


def f32_of(t64):
    """fp64 oracle values -> fp32 (exact mode: no rounding; zeros as +0)."""
    f = (t64 + 0.0).float()
    assert bool((f.double() == t64).all())
    return f


def bf16_of(bits):
    return uo.bits_to_bf16(bits)


class Arena:
    """p, g, buf of one launch target, each guarded."""

    def __init__(self, n, seed, exact=True):
        self.n, self.exact, self.seed = n, exact, seed
        self.p, self.g, self.buf = Buf(n), Buf(n), Buf(n)
        self.p.set(self._draw(seed))
        self.buf.set(self._draw(seed + 1))
        self.new_grad(0)

    def _draw(self, seed):
        if self.exact:
            return int_tensor((self.n,), -64, 64, seed)
        return torch.randn(self.n, generator=torch.Generator().manual_seed(seed))

    def new_grad(self, step):
        self.g.set(self._draw(self.seed + 2 + step))

    def host64(self):
        return tuple(b.inner.cpu().double() for b in (self.p, self.g, self.buf))


def descs_tensor(rows):
    return torch.tensor(rows if rows else [[0] * 12], dtype=torch.int64, device=DEV)


def launch(nat, items, rows, A, h, lr_arg=None, **kw):
    """One sgd_pack launch; ``lr_arg``: the immediate rate handed to the kernel when it differs
    from the one in force (a schedule is attached and must be read instead)."""
    it = torch.tensor(items, dtype=torch.int32, device=DEV)
    ds = descs_tensor(rows)
    nat.sgd_pack(it.data_ptr(), len(items), ds.data_ptr(), A.p.ptr, A.g.ptr, A.buf.ptr,
                 h["lr"] if lr_arg is None else lr_arg, h["momentum"], h["wd"], h["grad_scale"],
                 int(h["nesterov"]), stream(),
                 zero_grad=int(h.get("zero_grad", 0)), delta=int(h.get("delta", 0)),
                 sched_advance=int(h.get("sched_advance", 0)), **kw)
    torch.cuda.synchronize()


def check_launch(nat, items, rows, A, h, steps, mem=None, shadow=None, slot=None, check_ties=False,
                 osched=None, ohyper=None, guard_skipped=False, **kw):
    """``steps`` launches of one table, each compared with the oracle: p, g, buf, every bf16 copy,
    shadow and slot, whole buffers. ``osched``: the oracle's image of the schedule the launch
    reads. ``ohyper``: the oracle's hyper-parameters where the launch's own guard changes them
    (grad_scale * c); ``guard_skipped``: the oracle runs the guard's skipped step (exact mode).
    Returns the last oracle state."""
    mem = mem or {}
    o = None
    for step in range(steps):
        if step:
            A.new_grad(step)
        before = {k: b.host() for k, b in dict(p=A.p, g=A.g, buf=A.buf, shadow=shadow, slot=slot,
                                               **{f"m{q}": b for q, b in mem.items()}).items()
                  if b is not None}
        p, g, buf = A.host64()
        okw = dict(mem={q: b.np_bits() for q, b in mem.items()},
                   shadow=None if shadow is None else shadow.np_bits(),
                   slot=None if slot is None else slot.inner.cpu().double(), sched=osched)
        launch(nat, items, rows, A, h, shadow=shadow.ptr if shadow else 0,
               slot=slot.ptr if slot else 0, **kw)
        if A.exact:
            o = uo.run_items(items, rows, p, g, buf, ohyper or h, exact=True,
                             guard_skipped=guard_skipped, **okw)
            same_bits(A.p.host(), A.p.expect(before["p"], f32_of(o["p"])), f"step {step}: p")
            same_bits(A.buf.host(), A.buf.expect(before["buf"], f32_of(o["buf"])),
                      f"step {step}: buf")
            if slot is not None:
                same_bits(slot.host(), slot.expect(before["slot"], f32_of(o["slot"])),
                          f"step {step}: slot")
            if check_ties and step == steps - 1:
                tie, odd = uo.is_tie(o["p"])
                assert (tie & ~odd).any() and odd.any(), "no bf16 ties of both parities"
        else:
            newp = A.p.inner.cpu().numpy()
            o = uo.run_items(items, rows, p, g, buf, h, pack_source=newp, **okw)
            t = uo.run_items(items, rows, p, g, buf, h, abs_pass=True, sched=osched)
            eps = FP32_EPS
            bp = torch.where(o["p"] == p, 0.0, r_p(h["nesterov"]) * eps * t["p"])
            bb = torch.where(o["buf"] == buf, 0.0, R_BUF * eps * t["buf"])
            wp = assert_within(A.p.inner.cpu(), o["p"], bp, what=f"step {step}: p")
            wb = assert_within(A.buf.inner.cpu(), o["buf"], bb, what=f"step {step}: buf")
            print(f"bound mode: worst |err|/bound p {wp:.3f} buf {wb:.3f}")
            for name, b in (("p", A.p), ("buf", A.buf)):
                got = b.host()
                same_bits(got, b.expect(before[name], got[GUARD:GUARD + b.n]), f"{name} guards")
            if slot is not None:  # the fp32 send slot holds the kernel's own new p
                want = before["slot"][GUARD:GUARD + slot.n].clone()
                for kind, a, cnt, so in items:
                    if kind == 3 and so >= 0:
                        want[so:so + cnt] = torch.from_numpy(newp[a:a + cnt])
                same_bits(slot.host(), slot.expect(before["slot"], want), "slot")
        same_bits(A.g.host(), A.g.expect(before["g"], f32_of(o["g"])), f"step {step}: g")
        for q, b in mem.items():
            same_bits(b.host(), b.expect(before[f"m{q}"], bf16_of(o["mem"][q])),
                      f"step {step}: bf16 copy {q}")
        if shadow is not None:
            same_bits(shadow.host(), shadow.expect(before["shadow"], bf16_of(o["shadow"])),
                      f"step {step}: shadow")
    return o


# ------------------------------------------------------------------------------------ sgd_kernel
BIG = 4 * 4096 * 256 + 4 * 300 + 3   # the only size that enters the grid-stride loop


def lr_sched(rates, step):
    """Device LrSched: int32 {step, n, next, pad} + n fp32 rates."""
    t = torch.zeros(4 + len(rates), dtype=torch.int32, device=DEV)
    t[:4] = torch.tensor([step, len(rates), step, 0], dtype=torch.int32)
    t[4:].view(torch.float32).copy_(torch.tensor(rates))
    return t


@pytest.mark.parametrize("n,nesterov,momentum,sched", [
    (n, nv, m, False) for n in (1, 3, 4, 5, 1023) for nv in (0, 1) for m in (0.5, 0.0)
] + [(BIG, 0, 0.5, False), (1023, 1, 0.5, True)])
def test_sgd_exact(native_ext, n, nesterov, momentum, sched):
    h = dict(EXACT, momentum=momentum, nesterov=nesterov)
    A = Arena(n, 100 + n % 97)
    table = lr_sched([2.0 ** -1, 2.0 ** -2, 2.0 ** -3], 1) if sched else None
    for step in range(2):
        if step:
            A.new_grad(step)
        before = [b.host() for b in (A.p, A.g, A.buf)]
        p, g, buf = A.host64()
        native_ext.sgd(A.p.ptr, A.g.ptr, A.buf.ptr, n, 99.0 if sched else h["lr"], momentum,
                       h["wd"], h["grad_scale"], nesterov, stream(),
                       sched=table.data_ptr() if sched else 0)
        torch.cuda.synchronize()
        rp, rb = uo.sgd_ref(p, g, buf, exact=True, **h)
        same_bits(A.p.host(), A.p.expect(before[0], f32_of(rp)), f"step {step}: p")
        same_bits(A.buf.host(), A.buf.expect(before[2], f32_of(rb)), f"step {step}: buf")
        same_bits(A.g.host(), before[1], f"step {step}: g")
        if momentum == 0.0:
            same_bits(A.buf.host(), before[2], "buf at momentum 0")
    if n >= 1023:
        tp, _ = uo.sgd_abs(p, g, buf, nesterov=nesterov, **EXACT)
        assert_exact(A.p.inner, rp, tp, what="p", unit=2.0 ** -13)
    if sched:
        assert table[:4].tolist() == [1, 3, 1, 0]  # the plain kernel reads, never advances


@pytest.mark.parametrize("nesterov", [0, 1])
def test_sgd_bound(native_ext, nesterov):
    n = 4 * 1024 + 3
    h = dict(PROJECT, nesterov=nesterov)
    A = Arena(n, 7, exact=False)
    before = [b.host() for b in (A.p, A.g, A.buf)]
    p, g, buf = A.host64()
    native_ext.sgd(A.p.ptr, A.g.ptr, A.buf.ptr, n, h["lr"], h["momentum"], h["wd"],
                   h["grad_scale"], nesterov, stream())
    torch.cuda.synchronize()
    rp, rb = uo.sgd_ref(p, g, buf, **h)
    tp, tb = uo.sgd_abs(p, g, buf, **h)
    assert_within(A.p.inner.cpu(), rp, r_p(nesterov) * FP32_EPS * tp, what="p")
    assert_within(A.buf.inner.cpu(), rb, R_BUF * FP32_EPS * tb, what="buf")
    same_bits(A.g.host(), before[1], "g")
    for b, w in ((A.p, before[0]), (A.buf, before[2])):
        got = b.host()
        same_bits(got, b.expect(w, got[GUARD:GUARD + n]), "guards")


# ---------------------------------------------------------------------------------------- item 0
def item0_table():
    """Counts {1, 3, 4, 5, 8191, 8192}, each at an offset that is a multiple of 4 and at one that
    is not, with unowned gaps between them."""
    items, off = [], 8
    for mis in (0, 1, 2, 3):
        for cnt in (1, 3, 4, 5, 8191, 8192):
            if mis in (2, 3) and cnt > 5:
                continue
            off = (off + 3) // 4 * 4 + mis
            items.append([0, off, cnt, 0])
            off += cnt + 5
    return items, off + 8


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("zero_grad", [0, 1])
def test_item0(native_ext, zero_grad, exact):
    items, n = item0_table()
    h = dict(EXACT if exact else PROJECT, nesterov=0, zero_grad=zero_grad)
    check_launch(native_ext, items, [], Arena(n, 11, exact), h, 2 if exact else 1,
                 check_ties=False)


@pytest.mark.parametrize("nesterov,momentum", [(1, 0.5), (0, 0.0), (1, 0.0)])
def test_item0_branches(native_ext, nesterov, momentum):
    items, n = item0_table()
    h = dict(EXACT, momentum=momentum, nesterov=nesterov)
    check_launch(native_ext, items, [], Arena(n, 12), h, 2)


# ---------------------------------------------------------------------------- items 2 and 5
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("K,C,R,krsc", [(20, 13, 1, 0), (12, 12, 3, 1)])
def test_item2_then_item5(native_ext, K, C, R, krsc, exact):
    """Item 2 (update + Wc in the master's order) and item 5 (Wc only) on one descriptor; the
    counts are multiples of 4 and not of 1024; two chunks, so the relative offset counts."""
    cnt = K * C * R * R
    assert cnt % 4 == 0 and cnt % 1024 != 0
    poff, n = 128, 128 + cnt + 64
    wc = Buf(cnt, torch.bfloat16)
    rows = [[poff, K, C, C, R, R, wc.ptr, 0, krsc, 0, 0, 0]]
    cut = 200 if cnt < 1024 else 1024
    h = dict(EXACT if exact else PROJECT, nesterov=0, zero_grad=1)
    A = Arena(n, 21, exact)
    items = [[2, 0, cut, 0], [2, cut, cnt - cut, 0]]
    check_launch(native_ext, items, rows, A, h, 2 if exact else 1, mem={wc.ptr: wc},
                 check_ties=exact and cnt > 1000)
    # the backward wrote new masters: item 5 re-packs them and touches nothing else
    A.p.set(A._draw(77) * (0.37 if not exact else 0.75))
    A.new_grad(5)
    before = {k: b.host() for k, b in dict(p=A.p, g=A.g, buf=A.buf, wc=wc).items()}
    items = [[5, 0, cut, 0], [5, cut, cnt - cut, 0]]
    launch(native_ext, items, rows, A, h)
    for k, b in dict(p=A.p, g=A.g, buf=A.buf).items():
        same_bits(b.host(), before[k], f"item 5: {k} untouched")
    want = uo.bf16_rne_bits(A.p.inner.cpu().numpy()[poff:poff + cnt])
    same_bits(wc.host(), wc.expect(before["wc"], bf16_of(want)), "item 5: Wc")


# ---------------------------------------------------------------------------------------- item 1
TILE_SHAPES = [(64, 3, 8, 3), (64, 3, 8, 7), (40, 40, 40, 3), (72, 32, 40, 3), (96, 80, 80, 1)]


def prefill(nat, A, row, wc, wt):
    """One pack_conv_weights call, as the library does before the first step; checked against
    the oracle's stand-alone pack; then the elements a tile item must (Wc pad channels) or must
    not (Wt rows c >= Cr) write are poisoned with the guard pattern."""
    poff, K, Cr, C, R, S = row[:6]
    bc, bt = wc.host(), wt.host() if wt else None
    nat.pack_conv_weights([(A.p.ptr + 4 * poff, wc.ptr, wt.ptr if wt else 0, K, Cr, C, R, S,
                            row[8])], stream())
    torch.cuda.synchronize()
    p32 = A.p.inner.cpu().numpy()
    ec, et = uo.pack_ref(p32, row, wc=np.zeros(wc.n, np.uint16) + 0x7fc5,
                         wt=np.zeros(wt.n, np.uint16) + 0x7fc5 if wt else None)
    same_bits(wc.host(), wc.expect(bc, bf16_of(ec)), "pack: Wc", (K, R, S, C),
              ("k", "r", "s", "c"))
    wc.inner.view(torch.int16).view(K, R, S, C)[..., Cr:] = 0x7fc5
    if wt:
        same_bits(wt.host(), wt.expect(bt, bf16_of(et)), "pack: Wt", (C, R, S, K),
                  ("c", "r", "s", "k"))
        wt.inner.view(torch.int16).view(C, R, S, K)[Cr:] = 0x7fc5


@pytest.mark.parametrize("with_wt", [0, 1])
@pytest.mark.parametrize("krsc", [0, 1])
@pytest.mark.parametrize("shape", TILE_SHAPES)
def test_item1_exact(native_ext, shape, krsc, with_wt):
    K, Cr, C, R = shape
    assert tuple(native_ext.sgd_tile_dims(R * R)) == uo.tile_dims(R * R)
    poff = 64
    A = Arena(poff + K * Cr * R * R + 64, 31)
    wc = Buf(K * R * R * C, torch.bfloat16)
    wt = Buf(C * R * R * K, torch.bfloat16) if with_wt else None
    row = [poff, K, Cr, C, R, R, wc.ptr, wt.ptr if wt else 0, krsc, 0, 0, 0]
    prefill(native_ext, A, row, wc, wt)
    mem = {wc.ptr: wc}
    if wt:
        mem[wt.ptr] = wt
    h = dict(EXACT, nesterov=0, zero_grad=1)
    o = check_launch(native_ext, uo.tile_items(0, row), [row], A, h, 2, mem=mem,
                     check_ties=K * Cr * R * R > 2000)
    got = wc.np_bits().reshape(K, R, R, C)
    assert (got[..., Cr:] == 0).all()                          # pad channels: +0
    if wt:
        assert (wt.np_bits().reshape(C, R, R, K)[Cr:] == 0x7fc5).all()  # never touched
    assert o is not None


@pytest.mark.parametrize("krsc", [0, 1])
def test_item1_bound(native_ext, krsc):
    K, Cr, C, R = 40, 40, 40, 3
    A = Arena(64 + K * Cr * R * R + 64, 32, exact=False)
    wc, wt = Buf(K * R * R * C, torch.bfloat16), Buf(C * R * R * K, torch.bfloat16)
    row = [64, K, Cr, C, R, R, wc.ptr, wt.ptr, krsc, 0, 0, 0]
    prefill(native_ext, A, row, wc, wt)
    check_launch(native_ext, uo.tile_items(0, row), [row], A, dict(PROJECT, nesterov=1), 1,
                 mem={wc.ptr: wc, wt.ptr: wt})


# ------------------------------------------------------------------------------- items 3 and 4
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("slot_off,with_shadow", [(8, 1), (-1, 1), (8, 0), (-1, 0)])
def test_items3_4(native_ext, slot_off, with_shadow, exact):
    """A shard of 4 * 300 elements (300 is no multiple of 256) and the gradient clear of the
    neighbouring range."""
    cnt, n = 1200, 64 + 1200 + 400 + 64
    A = Arena(n, 41, exact)
    shadow = Buf(n, torch.bfloat16) if with_shadow else None
    slot = Buf(8 + cnt + 8, fill=torch.full((8 + cnt + 8,), -3.0))
    items = [[3, 64, cnt, slot_off], [4, 64 + cnt, 400, 0]]
    h = dict(EXACT if exact else PROJECT, nesterov=0, zero_grad=1)
    check_launch(native_ext, items, [], A, h, 2 if exact else 1, shadow=shadow, slot=slot)


# ----------------------------------------------------------------------------------- mixed table
def mixed_table():
    """At least 300 items of every kind over one arena. Returns items, descriptor rows (bf16
    pointers filled in by the caller: entries 6 / 7 hold the element counts here), arena size,
    slot size."""
    rows, items, off = [], [], 64

    def conv(K, Cr, C, R, krsc, wt):
        nonlocal off
        rows.append([off, K, Cr, C, R, R, K * R * R * C, C * R * R * K if wt else 0, krsc, 0, 0, 0])
        off += (K * Cr * R * R + 63) // 64 * 64
        return len(rows) - 1

    d0 = conv(64, 3, 8, 3, 0, True)
    d1 = conv(40, 40, 40, 3, 1, True)
    d2 = conv(64, 64, 64, 1, 0, False)
    d3 = conv(16, 16, 16, 3, 1, False)
    items += uo.tile_items(d0, rows[d0]) + uo.tile_items(d1, rows[d1])
    items += [[2, s, 64, d2] for s in range(0, 64 * 64, 64)]
    items += [[5, s, 36, d3] for s in range(0, 16 * 16 * 9, 36)]
    rng = np.random.RandomState(3)
    for _ in range(200):
        cnt = int(rng.randint(1, 41))
        off += int(rng.randint(0, 7))
        items.append([0, off, cnt, 0])
        off += cnt
    off = (off + 63) // 64 * 64
    soff = 0
    for j in range(10):
        items.append([3, off, 64, soff if j % 2 == 0 else -1])
        soff += 64 if j % 2 == 0 else 0
        items.append([4, off + 64, 32, 0])
        off += 128
    order = rng.permutation(len(items))
    return [items[i] for i in order], rows, off + 64, soff + 8


class MixedCase:
    """mixed_table() on the device: arena, bf16 copies (prefilled and poisoned), shadow, slot,
    control words {counter, done ticket, signal, -} and a schedule at step 1 of 3. The kernel gets
    lr = 99 as its immediate argument: with a schedule attached it must read the table's entry
    of step 1, as the oracle does."""

    def __init__(self, nat, exact, zero_grad=1):
        self.items, self.rows, n, nslot = mixed_table()
        assert len(self.items) >= 300 and {it[0] for it in self.items} == {0, 1, 2, 3, 4, 5}
        self.A = Arena(n, 51, exact)
        self.mem = {}
        for r in self.rows:
            wc = Buf(r[6], torch.bfloat16)
            wt = Buf(r[7], torch.bfloat16) if r[7] else None
            r[6], r[7] = wc.ptr, wt.ptr if wt else 0
            prefill(nat, self.A, r, wc, wt)
            self.mem[wc.ptr] = wc
            if wt:
                self.mem[wt.ptr] = wt
        self.shadow = Buf(n, torch.bfloat16)
        self.slot = Buf(nslot, fill=torch.full((nslot,), -3.0))
        self.ctl = Buf(4, torch.int32, fill=torch.tensor([10, 0, 7, 0], dtype=torch.int32))
        ptr, self.cb = self.ctl.ptr, self.ctl.host()
        self.sched = lr_sched([0.5, 2.0 ** -2 if exact else 0.1, 0.125], 1)
        self.h = dict(EXACT if exact else PROJECT, nesterov=0, zero_grad=zero_grad, delta=3,
                      sched_advance=1)
        self.h["lr"] = uo.f32(self.h["lr"])
        self.kw = dict(counter=ptr, done=ptr + 4, signal=ptr + 8, sched=self.sched.data_ptr())
        self.osched = dict(step=1, n=3, next=1, rates=[0.5, self.h["lr"], 0.125])
        self.launches = 0

    def check(self, nat, steps, **kw):
        """``steps`` launches through check_launch, then the control words: the ticket reset by
        every launch, the counter and the signal raised, next == step + 1 (nothing commits it)."""
        o = check_launch(nat, self.items, self.rows, self.A, self.h, steps, mem=self.mem,
                         shadow=self.shadow, slot=self.slot, osched=self.osched, lr_arg=99.0,
                         **self.kw, **kw)
        self.launches += steps
        self.check_control("control")
        return o

    def check_control(self, what):
        want = [10 + 3 * self.launches, 0, 7 + self.launches, 0]
        same_bits(self.ctl.host(), self.ctl.expect(self.cb, torch.tensor(want, dtype=torch.int32)),
                  what)
        assert self.sched[:4].tolist() == [1, 3, 2, 0]

    def check_skip_word(self, nat, extra=None, **kw):
        """Skip word set: nothing but the counter, the signal and the staged step may change
        (``extra``: further buffers that must stay as they are)."""
        skip = torch.ones(1, dtype=torch.int32, device=DEV)
        self.A.new_grad(9)
        bufs = dict(p=self.A.p, g=self.A.g, buf=self.A.buf, shadow=self.shadow, slot=self.slot,
                    **{str(k): b for k, b in self.mem.items()}, **(extra or {}))
        before = {k: b.host() for k, b in bufs.items()}
        self.sched[2] = 1
        launch(nat, self.items, self.rows, self.A, self.h, lr_arg=99.0, shadow=self.shadow.ptr,
               slot=self.slot.ptr, skip=skip.data_ptr(), **self.kw, **kw)
        self.launches += 1
        for k, b in bufs.items():
            same_bits(b.host(), before[k], f"skipped launch: {k}")
        self.check_control("control after the skipped launch")


@pytest.mark.parametrize("exact", [True, False])
def test_mixed_table(native_ext, exact):
    m = MixedCase(native_ext, exact)
    m.check(native_ext, 2 if exact else 1, check_ties=exact)
    m.check_skip_word(native_ext)


def guard_buffers(partials, skipped=5):
    """The guard's device inputs: per-chunk partial sums and the statistics words {norm, c,
    skipped steps, -} (as int32 bit patterns), both between guard bands."""
    part = Buf(len(partials), fill=torch.tensor(partials))
    stats = Buf(4, torch.int32, fill=torch.tensor([0x11111111, 0x22222222, skipped, 0x44444444],
                                                  dtype=torch.int32))
    return part, stats


def f32_bits(x):
    return int(np.array([x], np.float32).view(np.int32)[0])


@pytest.mark.parametrize("zero_grad", [0, 1], ids=["zero_grad=0", "zero_grad=1"])
def test_mixed_table_guard_skipped(native_ext, zero_grad):
    """A non-finite norm with skip_nonfinite (clip flag 2) through the raw table: items 0-3 only
    clear their gradient range (with zero_grad), exactly the range the update covers -- whole
    guarded buffers against the oracle; items 4 and 5, the counter, the signal and the staged
    step as in any step; the statistics hold norm = +inf and c (1.0 without the clip flag,
    2 / (inf + eps) = 0.0 with it) and the skipped count goes up by one."""
    m = MixedCase(native_ext, True, zero_grad)
    part, stats = guard_buffers([1.0, float("inf"), 1.0])
    pb, sb = part.host(), stats.host()
    ckw = dict(clip_partial=part.ptr, clip_chunks=3, clip_max_norm=2.0, clip_eps=1e-6,
               clip_stats=stats.ptr)
    count = 5
    for flags in ((2 | 4, 1 | 2 | 4) if zero_grad else (2 | 4,)):
        m.A.new_grad(20 + flags)
        m.check(native_ext, 1, guard_skipped=True, clip_flags=flags, **ckw)
        count += 1
        want = [f32_bits(float("inf")), f32_bits(0.0 if flags & 1 else 1.0), count, 0x44444444]
        same_bits(stats.host(), stats.expect(sb, torch.tensor(want, dtype=torch.int32)),
                  f"statistics, flags {flags}")
        same_bits(part.host(), pb, "partials")
    # the skip word keeps precedence: nothing is touched and nothing recorded
    stats.set(torch.tensor([0x11111111, 0x22222222, count, 0x44444444], dtype=torch.int32))
    m.check_skip_word(native_ext, extra=dict(stats=stats, partials=part), clip_flags=2 | 4, **ckw)


def test_mixed_table_clip_half(native_ext):
    """Partials {4, 0, 12}: norm = sqrt(16) = 4, c = 2 / (4 + 0) = 0.5, all exact. One exact-mode
    step must equal the oracle's unguarded run with grad_scale 2**-1 * 0.5 = 2**-2 (the oracle
    asserts that every intermediate is an fp32 number); the statistics hold {4.0, 0.5} and the
    skipped count stays."""
    m = MixedCase(native_ext, True)
    part, stats = guard_buffers([4.0, 0.0, 12.0])
    pb, sb = part.host(), stats.host()
    m.check(native_ext, 1, ohyper=dict(m.h, grad_scale=2.0 ** -2),
            clip_partial=part.ptr, clip_chunks=3, clip_max_norm=2.0, clip_eps=0.0,
            clip_flags=1 | 2 | 4, clip_stats=stats.ptr)
    want = [f32_bits(4.0), f32_bits(0.5), 5, 0x44444444]
    same_bits(stats.host(), stats.expect(sb, torch.tensor(want, dtype=torch.int32)), "statistics")
    same_bits(part.host(), pb, "partials")


# ------------------------------------------------------------------------------ pack_conv_weights
def _pack_case(nat, shapes, seed):
    g0 = torch.Generator().manual_seed(seed)
    descs, bufs = [], []
    for (K, Cr, C, R, krsc, with_wt) in shapes:
        w = Buf(K * Cr * R * R, fill=torch.randn(K * Cr * R * R, generator=g0))
        wc = Buf(K * R * R * C, torch.bfloat16)
        wt = Buf(C * R * R * K, torch.bfloat16) if with_wt else None
        descs.append((w.ptr, wc.ptr, wt.ptr if wt else 0, K, Cr, C, R, R, krsc))
        bufs.append((w, wc, wt))
    before = [(w.host(), wc.host(), wt.host() if wt else None) for w, wc, wt in bufs]
    nat.pack_conv_weights(descs, stream())
    torch.cuda.synchronize()
    for (K, Cr, C, R, krsc, with_wt), (w, wc, wt), b in zip(shapes, bufs, before):
        row = [0, K, Cr, C, R, R, 1, 2, krsc]
        ec, et = uo.pack_ref(w.inner.cpu().numpy(), row, wc=np.zeros(wc.n, np.uint16),
                             wt=np.zeros(wt.n, np.uint16) if wt else None)
        same_bits(w.host(), b[0], "master untouched")
        same_bits(wc.host(), wc.expect(b[1], bf16_of(ec)), f"Wc {K}x{Cr}({C})x{R} krsc {krsc}",
                  (K, R, R, C), ("k", "r", "s", "c"))
        if wt:
            same_bits(wt.host(), wt.expect(b[2], bf16_of(et)), f"Wt {K}x{Cr}({C})x{R}",
                      (C, R, R, K), ("c", "r", "s", "k"))


def test_pack_65_descriptors(native_ext):
    """More than kMaxPack = 64 descriptors: the second launch carries the 65th."""
    base = [(8, 3, 8, 3, 0, 1), (16, 5, 8, 1, 0, 0), (8, 8, 8, 3, 1, 1), (24, 3, 8, 3, 1, 1),
            (8, 12, 16, 1, 1, 0), (16, 3, 8, 5, 0, 1), (8, 7, 8, 2, 1, 0)]
    _pack_case(native_ext, [base[i % len(base)] for i in range(65)], 61)


@pytest.mark.parametrize("krsc", [0, 1])
def test_pack_grid_stride(native_ext, krsc):
    """128 x 128 x 3 x 3 = 147456 elements, above the 512 blocks x 256 threads of one sweep;
    Cr = 120 of C = 128 (padding) with Wt."""
    _pack_case(native_ext, [(128, 120, 128, 3, krsc, 1)], 62 + krsc)


# -------------------------------------------------------------------------------------- shard_tail
TAIL_COUNTS = (0, 1, 255, 256, 257, 1001)


@pytest.mark.parametrize("n_pack,with_signal,skip,segs_on", [
    (0, 1, 0, 1), (1, 1, 0, 1), (4, 1, 0, 1), (4, 0, 0, 1), (1, 0, 0, 0), (1, 1, 0, 0),
    (4, 1, 1, 1), (1, 0, 1, 1)])
def test_shard_tail(native_ext, n_pack, with_signal, skip, segs_on):
    """Segments of {0, 1, 255, 256, 257, 1001} floats, two of them from overlapping source
    ranges, into an arena whose channel-padded conv masters (K = 16, Cr = 3 of C = 8, 3x3) the
    segments complete; then their Wc."""
    g0 = torch.Generator().manual_seed(71)
    K, Cr, C, R = 16, 3, 8, 3
    wn = K * Cr * R * R   # 432
    n = 64 + 4 * 448 + 2048
    dst = Buf(n, fill=torch.randn(n, generator=g0))
    src = Buf(2048, fill=torch.randn(2048, generator=g0))
    segs, d = [], 64 + 4 * 448
    for j, cnt in enumerate(TAIL_COUNTS):
        segs.append([37 * j, d, cnt, 0])   # sources overlap: 37 * j + cnt > 37 * (j + 1)
        d += cnt + 3
    rows, mem = [], {}
    for q in range(n_pack):
        wc = Buf(K * R * R * C, torch.bfloat16)
        off = 64 + q * 448
        rows.append([off, K, Cr, C, R, R, wc.ptr, 0, q % 2, 0, 0, 0])
        mem[wc.ptr] = wc
        segs.append([1000 + q * 8, off, wn, 0])   # the master itself arrives by a segment
    if not segs_on:
        segs = []
    ctl = Buf(4, torch.int32, fill=torch.tensor([0, 5, skip, 0], dtype=torch.int32))
    cb = ctl.host()
    table = torch.tensor(segs if segs else [[0, 0, 0, 0]], dtype=torch.int32, device=DEV)
    before = dst.host()
    mbefore = {k: b.host() for k, b in mem.items()}
    native_ext.shard_tail(table.data_ptr(), len(segs), src.ptr, dst.ptr,
                          [(dst.ptr + 4 * r[0], r[6], 0, K, Cr, C, R, R, r[8]) for r in rows],
                          ctl.ptr, ctl.ptr + 4 if with_signal else 0, ctl.ptr + 8, stream())
    torch.cuda.synchronize()
    ed, em, done, sig = uo.shard_tail_ref(segs, src.inner.cpu().numpy(),
                                          before[GUARD:GUARD + n].numpy(), rows,
                                          mem={k: uo.bf16_to_bits(mbefore[k][GUARD:-GUARD])
                                               for k in mem},
                                          signal=5 if with_signal else None, skip=skip)
    same_bits(dst.host(), dst.expect(before, torch.from_numpy(ed)), "dst")
    for k, b in mem.items():
        same_bits(b.host(), b.expect(mbefore[k], bf16_of(em[k])), "tail Wc", (K, R, R, C),
                  ("k", "r", "s", "c"))
    want = [0, 6 if with_signal else 5, skip, 0]
    same_bits(ctl.host(), ctl.expect(cb, torch.tensor(want, dtype=torch.int32)), "control")
    assert done == 0 and sig == (6 if with_signal else None)


def test_shard_tail_five_packs_raises(native_ext):
    w, wc, ctl = Buf(64), Buf(64, torch.bfloat16), Buf(4, torch.int32)
    table = torch.zeros(1, 4, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        native_ext.shard_tail(table.data_ptr(), 0, w.ptr, w.ptr,
                              [(w.ptr, wc.ptr, 0, 8, 1, 8, 1, 1, 0)] * 5, ctl.ptr, 0, 0, stream())
    torch.cuda.synchronize()
    same_bits(wc.host(), Buf(64, torch.bfloat16).host(), "Wc after the refused call")


# -------------------------------------------------------------------------------------- lars_norms
def test_lars_norms_exact(native_ext):
    """Integers in [-8, 8], grad_scale 2**-1: every square and partial sum is a multiple of 1/4
    below 2**24, so the partials equal the integer sums whatever the reduction order."""
    counts = (1, 3, 4, 5, 8191, 8192)
    slots = (4, 0, 5, 2, 1, 7)          # chunk numbers: slots 3 and 6 stay unwritten
    offs, off = [], 8
    for c in counts:
        offs.append(off)
        off = (off + c + 7) // 4 * 4
    n = off + 8
    p = Buf(n, fill=int_tensor((n,), -8, 8, 81))
    g = Buf(n, fill=int_tensor((n,), -8, 8, 82))
    part = Buf(16)
    items = torch.tensor([[o, c, s, 0] for o, c, s in zip(offs, counts, slots)], dtype=torch.int32,
                         device=DEV)
    before, pb, gb = part.host(), p.host(), g.host()
    native_ext.lars_norms(items.data_ptr(), len(counts), p.ptr, g.ptr, 0.5, part.ptr, stream())
    torch.cuda.synchronize()
    ph, gh = p.inner.cpu().double(), g.inner.cpu().double()
    want = before[GUARD:GUARD + 16].clone().view(8, 2)
    got = part.inner.cpu().view(8, 2)
    for o, c, s in zip(offs, counts, slots):
        sp = (ph[o:o + c] ** 2).sum().reshape(1)
        sg = ((gh[o:o + c] * 0.5) ** 2).sum().reshape(1)
        assert_exact(got[s, 0:1], sp, sp, what=f"sum p^2, count {c}")
        assert_exact(got[s, 1:2], sg, sg, what=f"sum (g gs)^2, count {c}", unit=0.25)
        want[s, 0], want[s, 1] = float(sp), float(sg)
    same_bits(part.host(), part.expect(before, want), "partials and the unwritten slots")
    same_bits(p.host(), pb, "p")
    same_bits(g.host(), gb, "g")


# ------------------------------------------------------------------- through the Python builders
def _int_like(t, seed):
    return int_tensor(tuple(t.shape), -64, 64, seed).to(t.device)


@pytest.mark.parametrize("shape,cpad", [((64, 3, 3, 3), 8), ((48, 40, 3, 3), None),
                                        ((256, 64, 1, 1), None)])
def test_fused_sgd_step_exact(native_ext, shape, cpad):
    """FusedSGD.step (the Python table builder + the arena's own layout) against the per-tensor
    formula: no table on the reference side at all."""
    from ddp_amd.ops.layers import ConvBNActSpec
    from ddp_amd.optim import FusedSGD
    K, Cr, R, S = shape
    conv = torch.nn.Conv2d(Cr, K, R, padding=R // 2).to(DEV)
    bn = torch.nn.BatchNorm2d(K).to(DEV)
    extra = torch.nn.Parameter(torch.zeros(8192 + 5, device=DEV))
    spec = ConvBNActSpec(conv, bn, cin_pad=cpad)
    params = list(conv.parameters()) + list(bn.parameters()) + [extra]
    opt = FusedSGD(params, momentum=EXACT["momentum"], weight_decay=EXACT["wd"], lr=EXACT["lr"],
                   grad_scale=EXACT["grad_scale"])
    with torch.no_grad():
        for i, p in enumerate(params):
            p.copy_(_int_like(p, 200 + i))
    spec.maybe_pack()
    ref = [(p.detach().cpu().double(), torch.zeros(p.shape, dtype=torch.float64)) for p in params]
    for step in range(2):
        opt.zero_grad()
        for i, p in enumerate(params):
            p.grad.copy_(_int_like(p, 300 + 10 * step + i))
        gs = [p.grad.detach().cpu().double() for p in params]
        opt.step()
        torch.cuda.synchronize()
        ref = [uo.sgd_ref(rp, g, rb, nesterov=0, exact=True, **EXACT)
               for (rp, rb), g in zip(ref, gs)]
        for i, (p, (rp, _)) in enumerate(zip(params, ref)):
            same_bits(p.detach().cpu().contiguous(), f32_of(rp), f"step {step}: parameter {i}",
                      guard=0)
    w = ref[0][0]
    C = spec.C
    ewc = torch.zeros(K, R, S, C, dtype=torch.float64)
    ewc[..., :Cr] = w.permute(0, 2, 3, 1)
    same_bits(spec.wc.cpu(), bf16_of(uo.bf16_bits_of(ewc)).view(K, R, S, C), "Wc", (K, R, S, C),
              ("k", "r", "s", "c"), guard=0)
    tie, odd = uo.is_tie(w)
    assert (tie & ~odd).any() and odd.any()


def test_step_elements_scalar_branch(native_ext):
    """step_elements(5, 5 + 2 * 8192 + 3): chunks that start off a multiple of 4 take the scalar
    branch of item 0; the elements outside the range are not touched."""
    from ddp_amd.optim import FusedSGD
    n = 3 * 8192
    lo, hi = 5, 5 + 2 * 8192 + 3
    prm = torch.nn.Parameter(int_tensor((n,), -64, 64, 91).to(DEV))
    opt = FusedSGD([prm], momentum=EXACT["momentum"], weight_decay=EXACT["wd"], lr=EXACT["lr"],
                   grad_scale=EXACT["grad_scale"])
    p, buf = prm.detach().cpu().double(), torch.zeros(n, dtype=torch.float64)
    for step in range(2):
        opt.zero_grad()
        prm.grad.copy_(int_tensor((n,), -64, 64, 92 + step))
        g = prm.grad.detach().cpu().double()
        opt.step_elements(lo, hi, zero_grad=True)
        torch.cuda.synchronize()
        p, buf = p.clone(), buf.clone()
        p[lo:hi], buf[lo:hi] = uo.sgd_ref(p[lo:hi], g[lo:hi], buf[lo:hi], nesterov=0, exact=True,
                                          **EXACT)
        g[lo:hi] = 0.0
        same_bits(opt.arena.data.cpu()[:n], f32_of(p), f"step {step}: p", guard=0)
        same_bits(opt.momentum_buffer.cpu()[:n], f32_of(buf), f"step {step}: buf", guard=0)
        same_bits(opt.arena.grad.cpu()[:n], f32_of(g), f"step {step}: g", guard=0)


def test_tile_overflow_is_refused(native_ext):
    """A tile-path conv whose TK x TC x R x S tile exceeds the kernel's LDS tile (9x9 first layer
    with channel padding: 8 * 16 * 81 floats) is refused by the table builder, by name, before
    anything is launched."""
    from ddp_amd.ops.layers import ConvBNActSpec
    from ddp_amd.optim import FusedSGD, LARS
    tk, tc = native_ext.sgd_tile_dims(81)
    assert tk * tc * 81 > native_ext.sgd_tile_limit() >= 32 * 32 * 9
    for cls in (FusedSGD, LARS):
        conv = torch.nn.Conv2d(3, 64, 9, padding=4).to(DEV)
        spec = ConvBNActSpec(conv, None, cin_pad=8)
        opt = cls(list(conv.parameters()), lr=0.1, momentum=0.9)
        for _ in range(2):   # refused every time, not only on the first build
            with pytest.raises(ValueError, match=r"parameter 0 \(conv weight 64x3x9x9"):
                opt._work_table()
        assert spec.C == 8
    # the largest filter the tile holds is still accepted: 8 * 16 * 72 = 9216
    conv = torch.nn.Conv2d(3, 64, (8, 9), padding=4).to(DEV)
    spec = ConvBNActSpec(conv, None, cin_pad=8)
    items, n_items, _ = FusedSGD(list(conv.parameters()), lr=0.1)._work_table()
    assert n_items > 0 and spec.R * spec.S == 72


# ------------------------------------------------------------------- SGD in the WGRAD finish
@pytest.mark.parametrize("path", ["pair", "separate", "layer0", "pair_unsplit"])
def test_sgd_in_backward_finish_exact(native_ext, path):
    """conv_igemm.hip SgdFuse, the exact companion of test_gpu_kernels.test_sgd_in_backward_finish
    (its paths, plus the unsplit WGRAD epilogue that updates the master only): the gradient inside
    the finish never reaches memory, so only the result can be checked -- bit for bit here.
    x and dz are integers in [-2, 2] (dw is an integer, its magnitudes sum to at most 4 * N * H * W
    = 32768), p0 and buf0 multiples of 2**-3 in [-1, 1], the exact hyperparameters: the oracle
    asserts that nothing rounds. When the update is taken, p, buf and Wc must equal the oracle."""
    import torch.nn.functional as F
    from ddp_amd.ops.layers import ConvBNActSpec, conv_backward
    nat = native_ext
    if path == "layer0":
        N, Cin, H, K, Creal, need_dx = 8, 8, 32, 64, 3, False
    else:
        N, Cin, H, K, Creal, need_dx = 8, 64, 16, 128, 64, True
    conv = torch.nn.Conv2d(Creal, K, 3, 1, 1, bias=True).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(int_tensor((K, Creal, 3, 3), -1, 1, 401))
    spec = ConvBNActSpec(conv, None, cin_pad=Cin)
    spec.maybe_pack()
    x = int_tensor((N, Creal, H, H), -2, 2, 402)
    dz = int_tensor((N, K, H, H), -2, 2, 403)
    xn = torch.zeros(N, H, H, Cin, device=DEV, dtype=torch.bfloat16)
    xn[..., :Creal] = x.permute(0, 2, 3, 1).to(torch.bfloat16)
    dzn = dz.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)
    # fp64 reference gradient and the same on the magnitudes (the assert_exact precondition)
    wr = torch.zeros(K, Creal, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wr, None, 1, 1).backward(dz.double())
    dw64 = wr.grad.detach()
    wa = torch.zeros(K, Creal, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().abs(), wa, None, 1, 1).backward(dz.double().abs())
    h = dict(EXACT, nesterov=0)
    mode = {"pair": 2, "separate": 0, "layer0": 3, "pair_unsplit": 2}[path]
    wc0 = spec.wc.clone()
    nat.conv_pair_mode(mode)
    if path == "pair":
        nat.conv_pair_force(1, 4)  # WGRAD split 4 ways: a single-group finish
    if path == "pair_unsplit":
        nat.conv_pair_force(1, 1)  # no split: the WGRAD epilogue itself takes the master update
    try:
        dw_plain = torch.zeros_like(conv.weight, memory_format=torch.channels_last)
        conv_backward(spec, xn, dzn, dw_plain, need_dx)
        torch.cuda.synchronize()
        p0 = (int_tensor((K, Creal, 3, 3), -8, 8, 404) / 8.0)
        buf0 = (int_tensor((K, Creal, 3, 3), -8, 8, 405) / 8.0)
        p = p0.to(DEV).contiguous(memory_format=torch.channels_last)
        buf = buf0.to(DEV).contiguous(memory_format=torch.channels_last)
        dw = torch.zeros_like(p)
        nat.sgd_fuse_register(dw.data_ptr(), p.data_ptr(), buf.data_ptr(), spec.wc.data_ptr(),
                              h["lr"], h["momentum"], h["wd"], h["grad_scale"], 0, clear=1)
        nat.sgd_fuse_begin()
        try:
            conv_backward(spec, xn, dzn, dw, need_dx)
            torch.cuda.synchronize()
            taken, master = nat.sgd_fuse_taken(), nat.sgd_fuse_taken_master()
        finally:
            nat.sgd_fuse_register(0, clear=1)
    finally:
        nat.conv_pair_mode(3)
        nat.conv_pair_force(0, 0)
    names = ("k", "c", "r", "s")
    assert_exact(dw_plain, dw64, wa.grad, names=names, what="unfused dw")
    if path == "pair":
        assert taken == [dw.data_ptr()]
    if path == "pair_unsplit":
        assert master == [dw.data_ptr()] and taken == []
    if not taken and not master:   # the finish did not qualify: the gradient was stored
        assert_exact(dw, dw64, wa.grad, names=names, what="stored dw")
        same_bits(p.cpu().contiguous(), p0, "p untouched", guard=0)
        return
    assert float(dw.abs().max()) == 0.0
    rp, rb = uo.sgd_ref(p0.double(), dw64, buf0.double(), exact=True, **h)
    tp, tb = uo.sgd_abs(p0.double(), wa.grad, buf0.double(), **h)
    assert_exact(p, rp, tp, names=names, what="p", unit=2.0 ** -8)
    assert_exact(buf, rb, tb, names=names, what="buf", unit=2.0 ** -6)
    wc = spec.wc.cpu().view(K, 3, 3, Cin)
    want = wc0.cpu().view(K, 3, 3, Cin).clone()
    if taken:   # the finish rewrites the bf16 forward operand; the pad channels keep their +0
        want[..., :Creal] = bf16_of(uo.bf16_bits_of(rp.permute(0, 2, 3, 1).contiguous())) \
            .view(K, 3, 3, Creal)
    same_bits(wc, want, "Wc", (K, 3, 3, Cin), ("k", "r", "s", "c"), guard=0)
