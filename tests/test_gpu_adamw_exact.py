"""The AdamW rule of the fused update launch (csrc/kernels/optim.hip, the ADAM instantiations of
sgd_pack_kernel; api.h AdamArgs) against the CPU oracle of tests/adamw_oracle.py, element for
element and bit for bit, on the item table of tests/test_gpu_ema_exact.py (every path: scalar,
float4, krsc and 1x1 kind-2 convs, the channel-padded kind-1 layer, a [K][C][R][S] master with
Wt cut at both edges) with its guard-band convention: 64 elements of a NaN pattern around p, g,
m, v, the EMA and every bf16 copy, WHOLE buffers compared.

Exact mode, one step from a crafted state in which nothing rounds (the oracle asserts it):
    g integer in +-[1, 64], stored as 2 g with grad_scale 2**-1;  a in {+-1, +-2, +-3}, b in {1, 2, 4}
    m = (2 a - 1) g,  v = (2 b^2 - 1) g^2,  p integer in [-64, 64]
    omb1 = beta2 = omb2 = 2**-1, eps = 0, table entry (a1, a2) = (2, 2**-1), lr = 2**-2, wd = 2**-3
so m' = a g, v' = b^2 g^2, sqrt = b |g|, den = b |g| / 2, u = +-2 a / b, p' = p - p / 32 - u / 2.
p, m, v and the bf16 copies (which round for real) must equal the oracle; with the guard at
c == 1 and with the EMA (decay 0.75, exact as in the EMA test) the same.

Bound mode: randn inputs, the default hyper-parameters, non-zero m and v history, the table
entry of t = 3. The oracle reads the same table, so the two table roundings are not counted:
    |m' err| <= 3 eps T_m,  |v' err| <= 4 eps v',  |p' err| <= eps (3 (1 + lw) |p| + 10 la T_m / den)
(derivation: tests/test_adamw_cpu.py test_cpu_path_against_real_arithmetic). The bf16 copies
must be bitwise the RNE of what the kernel stored.
"""
import numpy as np
import pytest
import torch

import adamw_oracle as ao
import test_gpu_ema_exact as ex
import test_gpu_update_exact as ux
import update_oracle as uo
from exactness import FP32_EPS, assert_within, int_tensor

pytestmark = pytest.mark.gpu

DEV = "cuda"
Buf, same_bits, f32_of = ux.Buf, ux.same_bits, ux.f32_of
EXACT_HP = dict(lr=2.0 ** -2, wd=2.0 ** -3, grad_scale=2.0 ** -1, omb1=0.5, beta2=0.5, omb2=0.5,
                eps=0.0, a1=2.0, a2=0.5)
# the layout oracle: uo.run_items with lr = 0 leaves p as it is, so it writes the bf16 copies
# of, and clears the gradient ranges behind, whatever new p it is given
IDENTITY = dict(lr=0.0, momentum=0.0, wd=0.0, grad_scale=1.0, nesterov=0)


def default_hp(t=3):
    a1, a2 = ao.bias64(0.9, 0.999, t)
    return ao.hyper(1e-3, 1e-2, 0.5, 0.9, 0.999, 1e-8, a1, a2)


class Case(ex.Case):
    """ema_table() on the device with a second-moment arena; exact: the crafted state."""

    def __init__(self, nat, exact, seed=71):
        super().__init__(nat, exact, seed)
        n = self.A.n
        if exact:
            g = int_tensor((n,), 1, 64, seed + 10) * (2 * int_tensor((n,), 0, 1, seed + 11) - 1)
            a = int_tensor((n,), 1, 3, seed + 12) * (2 * int_tensor((n,), 0, 1, seed + 13) - 1)
            b = 2.0 ** int_tensor((n,), 0, 2, seed + 14)
            self.g_int = g
            self.A.g.set(2 * g)
            self.A.buf.set((2 * a - 1) * g)
            self.V = Buf(n, fill=(2 * b * b - 1) * g * g)
        else:
            gen = torch.Generator().manual_seed(seed + 15)
            self.A.buf.set(0.1 * torch.randn(n, generator=gen))
            self.V = Buf(n, fill=0.02 * torch.rand(n, generator=gen) + 1e-6)

    def buffers(self):
        return dict(super().buffers(), v=self.V)


def tables(hp, step=2, n_lr=4, n_bias=None):
    """Device LrSched and bias table whose entry of ``step`` holds hp's lr and {a1, a2}; the other
    entries hold values that would show (a clamp or an index slip fails the comparison)."""
    n_bias = n_bias or step + 2
    rates = [7.0 + i for i in range(n_lr)]
    rates[min(step, n_lr - 1)] = hp["lr"]
    bias = torch.tensor([[3.0 + i, 5.0 + i] for i in range(n_bias)], dtype=torch.float32)
    bias[min(step, n_bias - 1)] = torch.tensor([hp["a1"], hp["a2"]])
    return ux.lr_sched(rates, step), bias.to(DEV)


def adam_kw(case, hp, sched, bias):
    return dict(sched=sched.data_ptr(), adam_v=case.V.ptr, adam_bias=bias.data_ptr(),
                adam_n_bias=bias.shape[0], adam_omb1=hp["omb1"], adam_beta2=hp["beta2"],
                adam_omb2=hp["omb2"], adam_eps=hp["eps"])


def launch(nat, case, hp, zero_grad=1, step=2, n_lr=4, n_bias=None, **kw):
    """One ADAM launch; lr, momentum and nesterov arguments that must not be read."""
    sched, bias = tables(hp, step, n_lr, n_bias)
    h = dict(lr=99.0, momentum=0.75, wd=hp["wd"], grad_scale=hp["grad_scale"], nesterov=1,
             zero_grad=zero_grad)
    ux.launch(nat, case.items, case.rows, case.A, h, **adam_kw(case, hp, sched, bias), **kw)
    assert sched[:4].tolist() == [step, n_lr, step, 0]   # the launch stages nothing unasked


def expected(case, before64, hp, zero_grad, pack_source=None, guard_skipped=False):
    """The oracle's state after one launch: dict p, g, m, v (fp64) and mem (bf16 bits)."""
    p, g, m, v = before64
    mk = case.mask
    P, M, V = p.clone(), m.clone(), v.clone()
    if not guard_skipped:
        P[mk], M[mk], V[mk] = ao.adamw_ref(p[mk], g[mk], m[mk], v[mk], hp, exact=case.exact)
    mem = {q: b.np_bits() for q, b in case.mem.items()}
    o = uo.run_items(case.items, case.rows, P, g, M, dict(IDENTITY, zero_grad=zero_grad),
                     mem=mem, pack_source=pack_source, guard_skipped=guard_skipped)
    assert bool((o["p"] == P).all())
    return dict(p=P, g=o["g"], m=M, v=V, mem=o["mem"])


def check(nat, case, hp, zero_grad=1, ema_decay=None, guard_skipped=False, ohp=None, **kw):
    """One launch against the oracle, whole buffers. ``ohp``: the oracle's hyper-parameters where
    the launch's guard changes them (grad_scale * c)."""
    A = case.A
    before = {k: b.host() for k, b in case.buffers().items()}
    b64 = (*A.host64(), case.V.inner.cpu().double())
    e64 = case.E.inner.cpu().double()
    if ema_decay is not None:
        kw = dict(kw, ema=case.E.ptr, ema_one_minus_decay=ex.omd_of(ema_decay))
    launch(nat, case, hp, zero_grad, **kw)
    got_p = A.p.inner.cpu()
    o = expected(case, b64, ohp or hp, zero_grad, guard_skipped=guard_skipped,
                 pack_source=None if case.exact else got_p.numpy())
    if case.exact:
        for name, buf, key in (("p", A.p, "p"), ("m", A.buf, "m"), ("v", case.V, "v")):
            same_bits(buf.host(), buf.expect(before["buf" if name == "m" else name],
                                             f32_of(o[key])), name)
        if not guard_skipped:
            assert bool((o["p"] != b64[0])[case.mask].any())
    else:
        T = ao.adamw_abs(b64[0], b64[1], b64[2], b64[3], hp)
        bd = ao.bounds(T, FP32_EPS)
        zero = torch.zeros_like(b64[0])
        for name, buf, key in (("p", A.p, "p"), ("m", A.buf, "m"), ("v", case.V, "v")):
            worst = assert_within(buf.inner.cpu(), o[key], torch.where(case.mask, bd[name], zero),
                                  what=name)
            print(f"bound mode: worst |err|/bound {name} {worst:.3f}")
            got = buf.host()
            same_bits(got, buf.expect(before["buf" if name == "m" else name],
                                      got[ux.GUARD:ux.GUARD + buf.n]), f"{name} guards")
    same_bits(A.g.host(), A.g.expect(before["g"], f32_of(o["g"])), "g")
    for q, b in case.mem.items():
        same_bits(b.host(), b.expect(before[f"bf16 copy {q}"], ux.bf16_of(o["mem"][q])),
                  f"bf16 copy {q}")
    if ema_decay is None or guard_skipped:
        same_bits(case.E.host(), before["ema"], "ema: not this launch's")
    elif case.exact:
        want = torch.where(case.mask, ex.ema_ref(e64, o["p"], ex.omd_of(ema_decay), exact=True),
                           e64)
        same_bits(case.E.host(), case.E.expect(before["ema"], f32_of(want)), "ema")
    else:  # the lerp of the kernel's own new p: two roundings behind it
        omd = ex.omd_of(ema_decay)
        want = torch.where(case.mask, ex.ema_ref(e64, got_p.double(), omd), e64)
        T = e64.abs() + omd * (got_p.double().abs() + e64.abs())
        assert_within(case.E.inner.cpu(), want, torch.where(case.mask, 2 * FP32_EPS * T, 0.0),
                      what="ema")
    return o


# ------------------------------------------------------------------------------------- exact
@pytest.mark.parametrize("ema", [0, 1], ids=["noema", "ema"])
@pytest.mark.parametrize("guard", [0, 1], ids=["plain", "guard"])
def test_adamw_exact(native_ext, guard, ema):
    """All four ADAM instantiations: p, m, v and every bf16 copy bit for bit; the guard at c == 1
    (norm 4 below max_norm 8) leaves the same bits and stores its statistics."""
    case = Case(native_ext, True)
    kw, keep = ex.variant(case, 0, guard)
    check(native_ext, case, EXACT_HP, ema_decay=0.75 if ema else None, **kw)
    case.pad_channels_are_zero()
    if guard:
        assert ux.f32_bits(1.0) == int(keep[-1][1].inner.cpu()[1])


def test_adamw_exact_keeps_the_gradient_without_zero_grad(native_ext):
    case = Case(native_ext, True, seed=72)
    o = check(native_ext, case, EXACT_HP, zero_grad=0)
    assert bool((o["g"] != 0).any())


def test_adamw_follows_the_clipped_gradient(native_ext):
    """Partials {4, 0, 12}: norm 4, c = 2 / 4 = 0.5: the rule runs with grad_scale 2**-2. The
    crafted state is exact for G = g only, so this is a bound-mode step whose oracle takes the
    clipped scale."""
    case = Case(native_ext, False, seed=73)
    ckw, bufs = ex.guard_kw([4.0, 0.0, 12.0], 2.0, 1 | 2 | 4)
    hp = default_hp()
    check(native_ext, case, hp, ohp=dict(hp, grad_scale=hp["grad_scale"] * 0.5), **ckw)
    assert int(bufs[1].inner.cpu()[1]) == ux.f32_bits(0.5)


def test_table_index_clamps_to_the_last_entries(native_ext):
    """step 9 with 4 learning rates and 3 bias entries: both indices clamp, each to its own
    table's last entry."""
    case = Case(native_ext, True, seed=74)
    check(native_ext, case, EXACT_HP, step=9, n_lr=4, n_bias=3)


# ------------------------------------------------------------------------------------- bound
@pytest.mark.parametrize("ema", [0, 1], ids=["noema", "ema"])
def test_adamw_bound(native_ext, ema):
    case = Case(native_ext, False, seed=75)
    check(native_ext, case, default_hp(3), ema_decay=0.999 if ema else None)


# -------------------------------------------------------------------- behaviour in the launch
@pytest.mark.parametrize("guard", [0, 1], ids=["plain", "guard"])
def test_skip_word_leaves_everything(native_ext, guard):
    case = Case(native_ext, True, seed=76)
    kw, keep = ex.variant(case, 0, guard)
    skip = torch.ones(1, dtype=torch.int32, device=DEV)
    before = {k: b.host() for k, b in case.buffers().items()}
    launch(native_ext, case, EXACT_HP, skip=skip.data_ptr(), ema=case.E.ptr,
           ema_one_minus_decay=0.25, **kw)
    for k, b in case.buffers().items():
        same_bits(b.host(), before[k], f"skip word set: {k}")


@pytest.mark.parametrize("zero_grad", [0, 1])
def test_guard_skipped_step_clears_g_only(native_ext, zero_grad):
    case = Case(native_ext, True, seed=77)
    ckw, bufs = ex.guard_kw([1.0, float("inf"), 1.0], 2.0, 2 | 4)
    check(native_ext, case, EXACT_HP, zero_grad=zero_grad, ema_decay=0.75, guard_skipped=True,
          **ckw)
    assert int(bufs[1].inner.cpu()[2]) == 6   # counted


def test_two_runs_are_bit_identical(native_ext):
    a, b = Case(native_ext, False, seed=78), Case(native_ext, False, seed=78)
    hp = default_hp()
    for c in (a, b):
        launch(native_ext, c, hp, ema=c.E.ptr, ema_one_minus_decay=ex.omd_of(0.999))
    for (k, x), y in zip(a.buffers().items(), b.buffers().values()):
        same_bits(x.host(), y.host(), k)


def test_without_adam_v_the_launch_is_the_sgd_launch(native_ext):
    """adam.v == null with every other AdamArgs field set: the existing oracle on the same table,
    two exact steps, and v untouched."""
    case = Case(native_ext, True, seed=79)
    case.A.new_grad(0)                      # the update_exact state: integers in [-64, 64]
    case.A.buf.set(case.A._draw(79 + 1))
    hp = EXACT_HP
    _, bias = tables(hp)
    vb = case.V.host()
    ux.check_launch(native_ext, case.items, case.rows, case.A,
                    dict(ux.EXACT, nesterov=0, zero_grad=1), 2, mem=case.mem, adam_v=0,
                    adam_bias=bias.data_ptr(), adam_n_bias=bias.shape[0], adam_omb1=0.5,
                    adam_beta2=0.5, adam_omb2=0.5, adam_eps=0.25)
    same_bits(case.V.host(), vb, "v")


def test_refused_argument_combinations(native_ext):
    """ADAM excludes LARS, and needs the schedule's step word and a bias table."""
    case = Case(native_ext, True, seed=80)
    before = {k: b.host() for k, b in case.buffers().items()}
    lkw, keep = ex.lars_unit(len(case.items))
    with pytest.raises(RuntimeError):
        launch(native_ext, case, EXACT_HP, **lkw)
    sched, bias = tables(EXACT_HP)
    kw = adam_kw(case, EXACT_HP, sched, bias)
    h = dict(ux.EXACT, nesterov=0)
    for bad in (dict(kw, sched=0), dict(kw, adam_bias=0), dict(kw, adam_n_bias=0)):
        with pytest.raises(RuntimeError):
            ux.launch(native_ext, case.items, case.rows, case.A, h, **bad)
    for k, b in case.buffers().items():
        same_bits(b.host(), before[k], f"refused launch: {k}")


# ------------------------------------------------------------------- through the Python class
def _rig(seed, **kw):
    """tests/test_gpu_ema_exact.py _rig with AdamW: two convs (tile items; item 2), BatchNorm
    vectors, a two-chunk vector; randn state with a history in m and v; EMA on."""
    from ddp_amd.ops.layers import ConvBNActSpec
    from ddp_amd.optim import AdamW
    torch.manual_seed(seed)
    c0 = torch.nn.Conv2d(3, 64, 3, padding=1).to(DEV)
    b0 = torch.nn.BatchNorm2d(64).to(DEV)
    c1 = torch.nn.Conv2d(64, 48, 3, padding=1).to(DEV)
    extra = torch.nn.Parameter(torch.randn(8192 + 5, device=DEV))
    specs = [ConvBNActSpec(c0, b0, cin_pad=8), ConvBNActSpec(c1, None)]
    params = list(c0.parameters()) + list(b0.parameters()) + list(c1.parameters()) + [extra]
    opt = AdamW(params, grad_scale=0.5, **kw)
    for sp in specs:
        sp.maybe_pack()
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    opt.momentum_buffer.copy_(0.1 * torch.randn(opt.arena.total, device=DEV, generator=g))
    opt.second_moment.copy_(0.02 * torch.rand(opt.arena.total, device=DEV, generator=g) + 1e-6)
    opt.arena.grad.copy_(torch.randn(opt.arena.total, device=DEV, generator=g))
    opt.set_ema(0.9)
    opt.set_lr_step(2)
    torch.cuda.synchronize()
    return params, specs, opt


def test_per_range_launches_equal_the_whole_launch_and_the_cpu_path(native_ext):
    """``step(params=...)`` over a 3-way partition -- what the pipelined step issues per bucket,
    every launch reading the same step word -- leaves the bits of one whole launch; t advanced
    once; and every parameter is within the bound of the oracle at t = 3."""
    pa, sa, oa = _rig(1)
    pb, sb, ob = _rig(1)
    state0 = [t.clone() for t in (oa.arena.data, oa.arena.grad, oa.momentum_buffer,
                                  oa.second_moment)]
    oa.step(zero_grad=True)
    n = len(pb)
    for rng in ((0, 2), (2, 5), (5, n)):
        ob.step(zero_grad=True, params=rng, lr_advance=(rng[1] == n))
    torch.cuda.synchronize()
    assert oa.lr_step == ob.lr_step == 3 == oa.lr_step_device() == ob.lr_step_device()
    for what, x, y in (("p", oa.arena.data, ob.arena.data), ("ema", oa.ema, ob.ema),
                       ("m", oa.momentum_buffer, ob.momentum_buffer),
                       ("v", oa.second_moment, ob.second_moment),
                       ("g", oa.arena.grad, ob.arena.grad)):
        same_bits(x.cpu(), y.cpu(), what, guard=0)
    for s, t in zip(sa, sb):
        same_bits(s.wc.cpu().reshape(-1), t.wc.cpu().reshape(-1), "Wc", guard=0)
    a1, a2 = oa.bias_at(2)
    assert (a1, a2) == tuple(uo.f32(x) for x in ao.bias64(0.9, 0.999, 3))
    hp = ao.hyper(1e-3, 1e-2, 0.5, 0.9, 0.999, 1e-8, a1, a2)
    a = oa.arena
    for i in range(n):
        sl = slice(a.offsets[i], a.offsets[i] + a.numels[i])
        p, g, m, v = (t[sl].cpu().double() for t in state0)
        want = ao.adamw_ref(p, g, m, v, hp)
        bd = ao.bounds(ao.adamw_abs(p, g, m, v, hp), FP32_EPS)
        for name, got, w in (("p", a.data, want[0]), ("m", oa.momentum_buffer, want[1]),
                             ("v", oa.second_moment, want[2])):
            assert_within(got[sl].cpu(), w, bd[name], what=f"parameter {i}: {name}")
        assert not bool(a.grad[sl].any()), f"parameter {i}: gradient not cleared"


def test_state_snapshot_restores_every_arena(native_ext):
    pa, sa, oa = _rig(2)
    want = [t.clone() for t in (oa.momentum_buffer, oa.second_moment, oa.ema)]
    ptrs = [t.data_ptr() for t in (oa.momentum_buffer, oa.second_moment, oa.ema)]
    snap = oa.state_snapshot()
    oa.step(zero_grad=True)
    torch.cuda.synchronize()
    assert oa.lr_step == 3 and not torch.equal(oa.second_moment, want[1])
    oa.restore_state(snap)
    torch.cuda.synchronize()
    assert oa.lr_step == 2 == oa.lr_step_device()
    for t, w, ptr in zip((oa.momentum_buffer, oa.second_moment, oa.ema), want, ptrs):
        assert torch.equal(t, w) and t.data_ptr() == ptr
