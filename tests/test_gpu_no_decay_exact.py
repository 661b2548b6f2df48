"""The no-decay flag of the fused update launch (csrc/kernels/optim.hip: bit 8 of an updating work
item's kind word, bit 0 of the fourth field of a LAMB norms item) in raw launches, against
tests/decay_oracle.py: flagged items take the launch's rule with wd = 0, their neighbours keep
the launch's wd, nothing else moves.

The harness is that of tests/test_gpu_update_exact.py -- 64-element guard bands of a NaN pattern
around every buffer, WHOLE buffers compared as integers, the ``EXACT`` hyper-parameters (lr 2**-2,
momentum 2**-1, wd 2**-3, grad_scale 2**-1, integer operands in [-64, 64], two steps) -- with its
oracle module replaced by one whose ``run_items`` understands the flag (``update_oracle`` itself
refuses a flagged kind, and stays as it is).

Bound mode (randn, the ``PROJECT`` hyper-parameters, once, on the kind-0 mix): |err| <= R * 2**-24
* T with T from the oracle's pass over the magnitudes with wd = 0 on the flagged items and R as
counted in tests/test_gpu_update_exact.py; an upper bound there, because fma(0, p, x) does not round.
"""
import pytest
import torch

import adamw_oracle as ao
import decay_oracle as do
import lamb_oracle as lo
import test_gpu_adamw_exact as gx
import test_gpu_ema_exact as ex
import test_gpu_lamb_exact as lx
import test_gpu_lars as gl
import test_gpu_update_exact as ux
import update_oracle as uo
from exactness import FP32_EPS, assert_within

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = do.NO_DECAY
Buf, same_bits = ux.Buf, ux.same_bits


class _FlagOracle:
    """update_oracle, with the ``run_items`` that splits a table by the flag."""
    run_items = staticmethod(do.run_items)

    def __getattr__(self, name):
        return getattr(uo, name)


@pytest.fixture(autouse=True)
def flag_oracle(monkeypatch):
    monkeypatch.setattr(ux, "uo", _FlagOracle())


# ------------------------------------------------------------------------------------ the tables
def kind0_mix(off=64):
    """In arena order, touching: an unflagged item of 5 elements (aligned start, scalar tail), a
    FLAGGED one of 7 (start with off & 3 == 1: the scalar path only), an unflagged tensor of 8196
    (two chunk items). Returns items and the first free offset."""
    assert off % 4 == 0
    items = [[0, off, 5, 0], [0 | F, off + 5, 7, 0], [0, off + 12, 8192, 0],
             [0, off + 12 + 8192, 4, 0]]
    return items, off + 12 + 8196


def full_table(with3=True):
    """The kind-0 mix, then FLAGGED items of every other updating kind with unflagged items of
    kinds 4 and 5 next to them. Descriptor rows carry the bf16 element counts in entries 6 / 7
    until the case allocates the copies.
      kind 1: every tile of a K 3, Cr 3, C 8, 3x3 conv stored [K][R][S][Cr] (the channel-padded
              layout: 81 masters, Wc 3 x 9 x 8 with +0 in the pad channels)
      kind 2: a 64-element 1x1 conv 8 -> 8 with its Wc;  kind 5: its twin, re-packed only
      kind 3: 64 elements with ``shadow`` and a send slot;  kind 4: the 64 behind them"""
    items, off = kind0_mix()
    off = (off + 63) // 64 * 64 + 64
    rows = []

    def conv(K, Cr, C, R, krsc):
        nonlocal off
        rows.append([off, K, Cr, C, R, R, K * R * R * C, 0, krsc, 0, 0, 0])
        off += (K * Cr * R * R + 63) // 64 * 64 + 64
        return len(rows) - 1

    d1, d2, d5 = conv(3, 3, 8, 3, 1), conv(8, 8, 8, 1, 0), conv(8, 8, 8, 1, 0)
    items += [[it[0] | F] + it[1:] for it in uo.tile_items(d1, rows[d1])]
    items += [[2 | F, 0, 64, d2], [5, 0, 64, d5]]
    if with3:
        items += [[3 | F, off, 64, 8], [4, off + 64, 64, 0]]
    off += 128 + 64
    return items, rows, off


class Case:
    """A table on the device: arena, EMA, second moment, bf16 copies (prefilled, pad channels
    poisoned), shadow and slot. ``mask``: the elements a launch updates; ``nodecay``: those a
    flagged item owns."""

    def __init__(self, nat, exact, seed, with3=True, rows_too=True):
        if rows_too:
            self.items, self.rows, n = full_table(with3)
        else:
            self.items, n = kind0_mix()
            self.rows, n = [], n + 64
        self.exact = exact
        self.A = ux.Arena(n, seed, exact)
        self.E = Buf(n, fill=self.A._draw(seed + 50))
        self.mem = {}
        for r in self.rows:
            wc = Buf(r[6], torch.bfloat16)
            r[6] = wc.ptr
            ux.prefill(nat, self.A, r, wc, None)
            self.mem[wc.ptr] = wc
        self.shadow = Buf(n, torch.bfloat16) if with3 and rows_too else None
        self.slot = Buf(8 + 64 + 8, fill=torch.full((80,), -3.0)) if with3 and rows_too else None
        plain = [do.strip(it) for it in self.items]
        self.mask = ex.updated_mask(plain, self.rows, n)
        self.nodecay = ex.updated_mask([do.strip(it) for it in self.items if do.flagged(it)],
                                       self.rows, n)
        assert bool(self.nodecay.any()) and bool((self.mask & ~self.nodecay).any())
        assert bool((self.mask | ~self.nodecay).all())

    def kw(self):
        return dict(mem=self.mem, shadow=self.shadow, slot=self.slot)


# ------------------------------------------------------------------ flagged next to unflagged
@pytest.mark.parametrize("zero_grad", [0, 1])
def test_neighbours_keep_their_own_decay(native_ext, zero_grad):
    """5 unflagged, 7 flagged, 8196 unflagged elements side by side, two exact steps: each item
    its own decay, the guards untouched. (Before the flag existed a flagged kind was unknown to
    the kernel's switch and its elements were not updated at all.)"""
    case = Case(native_ext, True, 211, rows_too=False)
    h = dict(ux.EXACT, nesterov=0, zero_grad=zero_grad)
    p0 = case.A.p.inner.cpu().double()
    o = ux.check_launch(native_ext, case.items, [], case.A, h, 2)
    assert bool((o["p"] != p0)[case.nodecay].any())
    # the two rules differ on these inputs: the oracle with the flags ignored is another state
    plain = uo.run_items([do.strip(it) for it in case.items], [], *case.A.host64(), h)
    again = do.run_items(case.items, [], *case.A.host64(), h)
    assert bool((plain["p"] != again["p"])[case.nodecay].any())
    assert bool((plain["p"] == again["p"])[~case.nodecay].all())


@pytest.mark.parametrize("nesterov,momentum", [(1, 0.5), (0, 0.0)])
def test_neighbours_branches(native_ext, nesterov, momentum):
    case = Case(native_ext, True, 212, rows_too=False)
    h = dict(ux.EXACT, momentum=momentum, nesterov=nesterov, zero_grad=1)
    ux.check_launch(native_ext, case.items, [], case.A, h, 2)


def test_neighbours_bound(native_ext):
    case = Case(native_ext, False, 213, rows_too=False)
    ux.check_launch(native_ext, case.items, [], case.A, dict(ux.PROJECT, nesterov=1), 1)


# ----------------------------------------------------- every updating kind, every instantiation
@pytest.mark.parametrize("variant", ["plain", "guard", "ema", "guard+ema"])
def test_flagged_items_of_every_kind_exact(native_ext, variant):
    """Flagged kinds 0, 1, 2 and 3 with unflagged kinds 0, 4 and 5 next to them, two exact steps,
    through the plain, GUARD (c == 1: norm 4 below max_norm 8) and EMA instantiations."""
    case = Case(native_ext, True, 221)
    assert {it[0] for it in case.items} == {0, 0 | F, 1 | F, 2 | F, 3 | F, 4, 5}
    kw, keep = ex.variant(case, 0, "guard" in variant)
    h = dict(ux.EXACT, nesterov=0, zero_grad=1)
    if "ema" in variant:
        ex.check_ema_launch(native_ext, case, h, 2, 0.75, shadow=case.shadow, slot=case.slot, **kw)
    else:
        ux.check_launch(native_ext, case.items, case.rows, case.A, h, 2, **case.kw(), **kw)
    r = case.rows[0]
    wc = case.mem[r[6]].np_bits().reshape(3, 3, 3, 8)
    assert (wc[..., 3:] == 0).all()   # the flagged tile items wrote +0 into the pad channels
    if "guard" in variant:
        assert ux.f32_bits(1.0) == int(keep[-1][1].inner.cpu()[1])


def test_flagged_items_follow_the_clipped_gradient(native_ext):
    """Partials {4, 0, 12}: norm 4, c = 2 / 4: every item, flagged or not, runs with grad_scale
    2**-2 and its own decay."""
    case = Case(native_ext, True, 222)
    ckw, bufs = ex.guard_kw([4.0, 0.0, 12.0], 2.0, 1 | 2 | 4)
    h = dict(ux.EXACT, nesterov=0, zero_grad=1)
    ux.check_launch(native_ext, case.items, case.rows, case.A, h, 1,
                    ohyper=dict(h, grad_scale=2.0 ** -2), **case.kw(), **ckw)
    assert int(bufs[1].inner.cpu()[1]) == ux.f32_bits(0.5)


@pytest.mark.parametrize("zero_grad", [0, 1])
def test_a_skipped_step_clears_the_flagged_items_gradients_like_the_others(native_ext, zero_grad):
    case = Case(native_ext, True, 223)
    ckw, bufs = ex.guard_kw([1.0, float("inf"), 1.0], 2.0, 2 | 4)
    h = dict(ux.EXACT, nesterov=0, zero_grad=zero_grad)
    g0 = case.A.g.inner.cpu().clone()
    ux.check_launch(native_ext, case.items, case.rows, case.A, h, 1, guard_skipped=True,
                    **case.kw(), **ckw)
    g1 = case.A.g.inner.cpu()
    if zero_grad:
        assert not bool(g1[case.mask].any()) and bool(g0[case.nodecay].any())
    assert int(bufs[1].inner.cpu()[2]) == 6   # counted


def test_skip_word_leaves_everything(native_ext):
    case = Case(native_ext, True, 224)
    skip = torch.ones(1, dtype=torch.int32, device=DEV)
    bufs = dict(p=case.A.p, g=case.A.g, buf=case.A.buf, shadow=case.shadow, slot=case.slot,
                **{str(k): b for k, b in case.mem.items()})
    before = {k: b.host() for k, b in bufs.items()}
    ux.launch(native_ext, case.items, case.rows, case.A, dict(ux.EXACT, nesterov=0, zero_grad=1),
              skip=skip.data_ptr(), shadow=case.shadow.ptr, slot=case.slot.ptr)
    for k, b in bufs.items():
        same_bits(b.host(), before[k], f"skip word set: {k}")


# ------------------------------------------------------------------------------------------ ADAM
@pytest.mark.parametrize("variant", ["plain", "guard", "ema"])
def test_adamw_flagged_items_within_the_oracles_bounds(native_ext, variant):
    """The ADAM instantiations on the table without kind 3 (compiled out there): randn state,
    default hyper-parameters at t = 3, per-element bounds of ``adamw_oracle.bounds`` with lw = 0
    on the flagged elements. The decay's own term, lr wd |p| = 1e-5 |p|, is two orders above the
    bound on p, so an element that took the wrong wd fails."""
    case = Case(native_ext, False, 231, with3=False)
    n = case.A.n
    gen = torch.Generator().manual_seed(232)
    case.A.buf.set(0.1 * torch.randn(n, generator=gen))
    case.V = Buf(n, fill=0.02 * torch.rand(n, generator=gen) + 1e-6)
    hp = gx.default_hp(3)
    kw, keep = ex.variant(case, 0, variant == "guard")
    if variant == "ema":
        kw = dict(kw, ema=case.E.ptr, ema_one_minus_decay=ex.omd_of(0.999))
    before = {k: b.host() for k, b in dict(p=case.A.p, g=case.A.g, m=case.A.buf, v=case.V).items()}
    mb = {q: b.host() for q, b in case.mem.items()}
    p, g, m = case.A.host64()
    v = case.V.inner.cpu().double()
    e64, eb = case.E.inner.cpu().double(), case.E.host()
    sched, bias = gx.tables(hp)
    h = dict(lr=99.0, momentum=0.75, wd=hp["wd"], grad_scale=hp["grad_scale"], nesterov=1, zero_grad=1)
    ux.launch(native_ext, case.items, case.rows, case.A, h, **gx.adam_kw(case, hp, sched, bias), **kw)
    mk = case.mask
    want = do.adamw_ref(p, g, m, v, hp, case.nodecay)
    bd = ao.bounds(do.adamw_abs(p, g, m, v, hp, case.nodecay), FP32_EPS)
    zero = torch.zeros_like(p)
    for name, buf, w, old in (("p", case.A.p, want[0], p), ("m", case.A.buf, want[1], m),
                              ("v", case.V, want[2], v)):
        worst = assert_within(buf.inner.cpu(), torch.where(mk, w, old),
                              torch.where(mk, bd[name], zero), what=name)
        print(f"{variant}: worst |err|/bound {name} {worst:.3f}")
        got = buf.host()
        same_bits(got, buf.expect(before[name], got[ux.GUARD:ux.GUARD + n]), f"{name} guards")
    decayed = ao.adamw_ref(p, g, m, v, hp)[0]
    apart = ((decayed - want[0]).abs() > 8 * bd["p"])[case.nodecay & (p.abs() > 0.1)]
    assert float(apart.float().mean()) > 0.9
    # the layout: gradients cleared behind, bf16 copies of, exactly what the kernel stored
    newp = case.A.p.inner.cpu()
    o = uo.run_items([do.strip(it) for it in case.items], case.rows, newp.double(), g, m,
                     dict(gx.IDENTITY, zero_grad=1), mem={q: b.np_bits() for q, b in case.mem.items()},
                     pack_source=newp.numpy())
    same_bits(case.A.g.host(), case.A.g.expect(before["g"], ux.f32_of(o["g"])), "g")
    for q, b in case.mem.items():
        same_bits(b.host(), b.expect(mb[q], ux.bf16_of(o["mem"][q])), f"bf16 copy {q}")
    if variant == "ema":
        omd = ex.omd_of(0.999)
        we = torch.where(mk, ex.ema_ref(e64, newp.double(), omd), e64)
        T = e64.abs() + omd * (newp.double().abs() + e64.abs())
        assert_within(case.E.inner.cpu(), we, torch.where(mk, 2 * FP32_EPS * T, 0.0), what="ema")
    else:
        same_bits(case.E.host(), eb, "ema: not this launch's")


# ---------------------------------------------------------------------------- LAMB: both kernels
@pytest.mark.parametrize("guarded", [False, True])
def test_lamb_norms_and_update_form_the_masked_direction_without_wd(native_ext, guarded):
    """tests/test_gpu_lamb_exact.py's chained rig with every tensor adapted and the 1-D ones
    masked: the norms launch (flag in its items) and the update launch (flag in the kind word)
    give a masked tensor the ratio |w| / |a1 u| within ``lamb_oracle.trust_rtol`` and p within
    ``lamb_oracle.bounds``; the unmasked tensors keep wd in both."""
    wd = 0.05
    kw = dict(max_grad_norm=1e9) if guarded else {}
    ps, specs, opt = lx._lamb_rig(weight_decay=wd, exclude_1d=False, no_decay="1d", **kw)
    masked = [p.dim() <= 1 for p in ps]
    assert opt.no_decay_mask == masked and sum(masked) == 5
    norm_items = opt._norm_table((0, len(ps)))[0].cpu()
    assert sorted(set(norm_items[:, 3].tolist())) == [0, 1]
    n = len(ps)
    state0 = [lx._views(opt, i) for i in range(n)]
    opt.step(zero_grad=True)
    torch.cuda.synchronize()
    a1, a2 = opt.bias_at(2)
    hp = ao.hyper(1e-3, wd, 0.5, 0.9, 0.999, 1e-8, a1, a2)
    stored = opt.trust_ratios().cpu()
    seen = 0
    for i in range(n):
        p, g, m, v = state0[i]
        h = dict(hp, wd=0.0) if masked[i] else hp
        r = lo.direction(p, g, m, v, h)[0]
        T = do.lamb_abs(p, g, m, v, hp, masked[i])
        want_t = lo.trust_of(lo.sum_sq(p), lo.sum_sq(r), True)
        got_t = float(stored[i])
        if want_t != 1.0:
            rtol = lo.trust_rtol(r, T["T_r"], FP32_EPS)
            print(f"parameter {i} masked {masked[i]}: trust {got_t!r} rel err "
                  f"{abs(got_t - want_t) / want_t:.3e} bound {rtol:.3e}")
            assert abs(got_t - want_t) <= rtol * want_t, i
            if masked[i]:   # the ratio WITH the wd term is elsewhere
                other = lo.trust_of(lo.sum_sq(p), lo.sum_sq(lo.direction(p, g, m, v, hp)[0]), True)
                assert abs(other - want_t) > 4 * rtol * want_t, i
                seen += 1
        else:
            assert got_t == 1.0, i
        want = do.lamb_ref(p, g, m, v, hp, masked[i], trust=got_t)
        bd = lo.bounds(T, FP32_EPS, hp["lr"] * got_t)
        got = lx._views(opt, i)
        for name, gt, w in (("p", got[0], want[0]), ("m", got[2], want[1]), ("v", got[3], want[2])):
            assert_within(gt.float(), w, bd[name], what=f"parameter {i}: {name}")
        assert not bool(got[1].any()), f"parameter {i}: gradient not cleared"
    assert seen >= 3   # conv bias, gamma, the 33-element vector (beta is 0: ratio 1)


# ------------------------------------------------------------------------------------------ LARS
def test_lars_masked_adapted_tensor_has_no_wd_term(native_ext):
    """tests/test_gpu_lars.py's tensors with every tensor adapted and the 1-D ones masked: the
    stored ratio is eta wn / (gn + eps) there and eta wn / (gn + wd wn + eps) elsewhere, within
    that file's TRUST_RTOL."""
    from ddp_amd.optim import LARS
    wd = 0.05
    ps, specs = gl._kernel_params()
    opt = LARS(ps, lr=0.3, momentum=gl.MOM, weight_decay=wd, grad_scale=gl.GS,
               trust_coefficient=gl.ETA, eps=gl.EPS, exclude_1d=False, no_decay="1d")
    gs = gl._grads(ps, 10)
    gl._set_grads(ps, gs)
    want, other = [], []
    for p, g in zip(ps, gs):
        wn, gn = float(p.detach().double().norm()), float((g.double() * gl.GS).norm())
        ok = wn > 0 and gn > 0
        w = 0.0 if p.dim() <= 1 else wd
        want.append(gl.ETA * wn / (gn + w * wn + gl.EPS) if ok else 1.0)
        other.append(gl.ETA * wn / (gn + wd * wn + gl.EPS) if ok else 1.0)
    opt.step()
    torch.cuda.synchronize()
    got = opt.trust_ratios().double().cpu()
    want, other = torch.tensor(want, dtype=torch.float64), torch.tensor(other, dtype=torch.float64)
    print("trust", got.tolist(), "want", want.tolist())
    assert torch.allclose(got, want, rtol=gl.TRUST_RTOL, atol=0.0), (got, want)
    far = (other - want).abs() > 100 * gl.TRUST_RTOL * want
    assert int(far.sum()) >= 3 and all(ps[i].dim() <= 1 for i in torch.nonzero(far).reshape(-1).tolist())
