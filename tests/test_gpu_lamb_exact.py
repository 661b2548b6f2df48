"""The LAMB kernels (csrc/kernels/optim.hip lamb_norms_kernel and the LAMB instantiations of
sgd_pack_kernel; api.h LambArgs, LambNorms) against the CPU oracle of tests/lamb_oracle.py, element
for element and bit for bit, on the item table and the guard-band convention of
tests/test_gpu_ema_exact.py / test_gpu_adamw_exact.py: 64 elements of a NaN pattern around every
buffer, WHOLE buffers compared.

Exact mode: AdamW's crafted state (test_gpu_adamw_exact.Case, EXACT_HP) with p drawn as multiples
of 8 in [-32, 32]: wd p and a1 u are integers, r is an integer with |r| <= 16, a chunk's sums stay
below 2^24 (the oracle asserts all of it). The update launch is handed a partial table written by
hand -- every tensor's sums are powers of four spread over its chunks, so wn, rn and the ratio
are powers of two (2^-1, 1, 2) -- as the BatchNorm exact tests hand their coefficient table in.

Bound mode, both kernels chained through optim.LAMB: randn inputs, default hyper-parameters, an
m and v history, t = 3, the parameter set of tests/test_gpu_lars.py. The ratios against fp64
within lamb_oracle.trust_rtol; p, m, v against the oracle run WITH THE RATIOS THE DEVICE STORED
within lamb_oracle.bounds (the two error sources stay apart); the bf16 copies bitwise.
"""
import numpy as np
import pytest
import torch

import adamw_oracle as ao
import lamb_oracle as lo
import test_gpu_adamw_exact as gx
import test_gpu_ema_exact as ex
import test_gpu_lars as gl
import test_gpu_update_exact as ux
import update_oracle as uo
from exactness import FP32_EPS, assert_within, int_tensor

pytestmark = pytest.mark.gpu

DEV = "cuda"
Buf, same_bits, f32_of = ux.Buf, ux.same_bits, ux.f32_of
EXACT_HP = gx.EXACT_HP


# ------------------------------------------------------------------------------ norms kernel
class NormsCase:
    """Three tensors between gaps: 8192 + 3000 elements (a full and a partial chunk), 330 (the
    scalar tail), 8192 (its chunk is NOT in the launch). Global chunks 1, 2, 3 and 5 of 7 slots."""
    SIZES = (8192 + 3000, 330, 8192)

    def __init__(self, exact, seed, gmul=2):
        self.exact = exact
        offs, off = [], 64
        for n in self.SIZES:
            offs.append(off)
            off += (n + 63) // 64 * 64 + 64
        n = off
        if exact:
            g = int_tensor((n,), 1, 64, seed) * (2 * int_tensor((n,), 0, 1, seed + 1) - 1)
            a = int_tensor((n,), 1, 3, seed + 2) * (2 * int_tensor((n,), 0, 1, seed + 3) - 1)
            b = 2.0 ** int_tensor((n,), 0, 2, seed + 4)
            vals = (8 * int_tensor((n,), -4, 4, seed + 5), gmul * g, (2 * a - 1) * g,
                    (2 * b * b - 1) * g * g)
        else:
            gen = torch.Generator().manual_seed(seed)
            vals = (torch.randn(n, generator=gen), torch.randn(n, generator=gen),
                    0.1 * torch.randn(n, generator=gen), 0.02 * torch.rand(n, generator=gen) + 1e-6)
        self.p, self.g, self.m, self.v = (Buf(n, fill=x) for x in vals)
        self.part = Buf(2 * 7)
        self.chunks = []   # (arena offset, count, global chunk)
        c = 1
        for o, sz in zip(offs, self.SIZES):
            for s0 in range(0, sz, 8192):
                self.chunks.append((o + s0, min(8192, sz - s0), c))
                c += 1
            c += 1 if sz == 330 else 0
        assert [c for _, _, c in self.chunks] == [1, 2, 3, 5]
        self.launched = self.chunks[:3]

    def bufs(self):
        return dict(p=self.p, g=self.g, m=self.m, v=self.v)

    def launch(self, nat, hp, **kw):
        sched, bias = gx.tables(hp)
        items = torch.tensor([[o, n, c, 0] for o, n, c in self.launched], dtype=torch.int32,
                             device=DEV)
        nat.lamb_norms(items.data_ptr(), len(self.launched), self.p.ptr, self.g.ptr, self.m.ptr,
                       hp["wd"], hp["grad_scale"], self.part.ptr, ux.stream(),
                       sched=sched.data_ptr(), adam_v=self.v.ptr, adam_bias=bias.data_ptr(),
                       adam_n_bias=bias.shape[0], adam_omb1=hp["omb1"], adam_beta2=hp["beta2"],
                       adam_omb2=hp["omb2"], adam_eps=hp["eps"], **kw)
        torch.cuda.synchronize()

    def want(self, hp):
        """The oracle's partial table: fp64 [7][2], NaN where the launch writes nothing."""
        w = torch.full((7, 2), float("nan"), dtype=torch.float64)
        host = [b.inner.cpu().double() for b in (self.p, self.g, self.m, self.v)]
        for o, n, c in self.launched:
            p, g, m, v = (t[o:o + n] for t in host)
            r = lo.direction(p, g, m, v, hp, exact=self.exact)[0]
            if self.exact:
                assert bool((r == r.round()).all()) and float(r.abs().max()) <= 16
            w[c] = torch.tensor([lo.sum_sq(p, self.exact), lo.sum_sq(r, self.exact)])
        return w


def _check_norms(nat, case, hp, ohp=None, **kw):
    before = {k: b.host() for k, b in case.bufs().items()}
    pb = case.part.host()
    want = case.want(ohp or hp)
    case.launch(nat, hp, **kw)
    for k, b in case.bufs().items():
        same_bits(b.host(), before[k], f"norms launch: {k} untouched")
    wrote = ~torch.isnan(want).reshape(-1)
    exp = pb[ux.GUARD:ux.GUARD + 14].clone()
    exp[wrote] = f32_of(want.reshape(-1)[wrote])
    same_bits(case.part.host(), case.part.expect(pb, exp), "partials")
    return case.part.host()


def test_norms_exact(native_ext):
    """Every float2 partial equals the fp64 oracle bit for bit; p, g, m, v are untouched and the
    slots of chunks outside the launch keep their NaN pattern."""
    _check_norms(native_ext, NormsCase(True, 91), EXACT_HP)


def _clip_kw(partials, max_norm):
    kw, keep = ex.guard_kw(partials, max_norm, 1 | 2 | 4)
    kw.pop("clip_stats")
    return kw, keep


def test_norms_under_the_guard(native_ext):
    """Clip partials {4, 0, 12}, max_norm 2: c = 2^-1. The gradient is stored as 4 g with grad_scale
    2^-1, so G = g at gs * c and the crafted state is exact there: the partials are the oracle's
    at grad_scale 2^-2. With c == 1 (max_norm 8) the bits are the unguarded kernel's."""
    case = NormsCase(True, 92, gmul=4)
    kw, keep = _clip_kw([4.0, 0.0, 12.0], 2.0)
    _check_norms(native_ext, case, EXACT_HP, ohp=dict(EXACT_HP, grad_scale=2.0 ** -2), **kw)
    a, b = NormsCase(True, 93), NormsCase(True, 93)
    kw, keep = _clip_kw([4.0, 0.0, 12.0], 8.0)
    got = _check_norms(native_ext, a, EXACT_HP, **kw)
    b.launch(native_ext, EXACT_HP)
    same_bits(got, b.part.host(), "c == 1 against the unguarded kernel")


def test_norms_bound(native_ext):
    """randn state, default hyper-parameters at t = 3: each chunk's sums within the chain's bound
    (33 + 6 + 3 additions of non-negative terms; sum r^2 with the roundings of r on top, as
    lamb_oracle.trust_rtol counts them)."""
    case = NormsCase(False, 94)
    hp = gx.default_hp(3)
    case.launch(native_ext, hp)
    got = case.part.inner.cpu().double().reshape(7, 2)
    host = [b.inner.cpu().double() for b in (case.p, case.g, case.m, case.v)]
    for o, n, c in case.launched:
        p, g, m, v = (t[o:o + n] for t in host)
        r = lo.direction(p, g, m, v, hp)[0]
        T = lo.lamb_abs(p, g, m, v, hp)
        sp, sr = lo.sum_sq(p), lo.sum_sq(r)
        amp = float((r.abs() * T["T_r"]).sum() / sr)
        assert abs(float(got[c, 0]) - sp) <= 42 * FP32_EPS * sp, c
        assert abs(float(got[c, 1]) - sr) <= (42 + 20 * amp) * FP32_EPS * sr, c
    assert bool(torch.isnan(got[[0, 4, 5, 6]]).all())


# --------------------------------------------------------------------- update launch, exact
class Case(gx.Case):
    """test_gpu_adamw_exact.Case with p in multiples of 8 (exact) and the LAMB tables: the seven
    tensors of ema_table() -- four convs, and plain tensors of 1, 7 and 8192 + 4 elements (two
    items) -- with hand-made partial sums."""
    #          d0   d1   d2   d3   1-elem            7-elem  two-item
    TRUST = (0.5, 1.0, 2.0, 0.5, 1.0, 2.0, 1.0)
    ADAPTED = (1, 1, 1, 1, 0, 1, 1)

    def __init__(self, nat, exact, seed=171):
        super().__init__(nat, exact, seed)
        n = self.A.n
        if exact:
            self.A.p.set(8 * int_tensor((n,), -4, 4, seed + 20))
        plain = sorted(it[1] for it in self.items if it[0] == 0)
        small = {plain[0]: 4, plain[1]: 5, plain[2]: 6, plain[3]: 6}

        def owner(it):
            return it[3] if it[0] == 2 else it[1] if it[0] == 1 else small[it[1]]
        self.owner = [owner(it) for it in self.items]
        seen, side = set(), []
        for t in self.owner:
            side.append([t, int(t not in seen)])
            seen.add(t)
        assert seen == set(range(7))
        self.side = torch.tensor(side, dtype=torch.int32, device=DEV)
        # three chunks per tensor from global chunk 3 t + 1; sums that are powers of four, spread
        sums = {0.5: ((4.0, 4.0, 8.0), (16.0, 16.0, 32.0)), 1.0: ((4.0, 4.0, 8.0), (8.0, 0.0, 8.0)),
                2.0: ((16.0, 16.0, 32.0), (4.0, 4.0, 8.0))}
        part = torch.full((3 * 7 + 2, 2), float("nan"))
        rows = []
        for t, (tr, ad) in enumerate(zip(self.TRUST, self.ADAPTED)):
            sp, sr = sums[tr] if t != 6 else ((0.0, 0.0, 0.0), (4.0, 4.0, 8.0))   # wn == 0: ratio 1
            if not ad:
                sp, sr = sums[2.0]                                                # must not be used
            part[3 * t + 1:3 * t + 4] = torch.tensor([sp, sr]).t()
            rows.append([3 * t + 1, 3, ad, 0])
        self.tensors = torch.tensor(rows, dtype=torch.int32, device=DEV)
        self.part = Buf(part.numel(), fill=part)
        self.trust = Buf(7)
        # per-element ratio of the arena
        self.ratio = torch.ones(n, dtype=torch.float64)
        for t, tr in enumerate(self.TRUST):
            mine = [it for it, o in zip(self.items, self.owner) if o == t]
            self.ratio[ex.updated_mask(mine, self.rows, n)] = tr

    def buffers(self):
        return dict(super().buffers(), lamb_partial=self.part, lamb_trust=self.trust)

    def lamb_kw(self):
        return dict(lamb_side=self.side.data_ptr(), lamb_tensors=self.tensors.data_ptr(),
                    lamb_partial=self.part.ptr, lamb_trust=self.trust.ptr)


def launch(nat, case, hp, zero_grad=1, **kw):
    gx.launch(nat, case, hp, zero_grad, **case.lamb_kw(), **kw)


def expected(case, before64, hp, zero_grad, guard_skipped=False):
    """The oracle's state after one exact launch (as test_gpu_adamw_exact.expected)."""
    p, g, m, v = before64
    mk = case.mask
    P, M, V = p.clone(), m.clone(), v.clone()
    if not guard_skipped:
        r, nm, nv = lo.direction(p[mk], g[mk], m[mk], v[mk], hp, exact=True)
        lt = hp["lr"] * case.ratio[mk]
        assert bool(uo.is_f32(lt).all())
        P[mk], M[mk], V[mk] = p[mk] - lt * r, nm, nv
        assert bool(uo.is_f32(P).all())
    mem = {q: b.np_bits() for q, b in case.mem.items()}
    o = uo.run_items(case.items, case.rows, P, g, M, dict(gx.IDENTITY, zero_grad=zero_grad),
                     mem=mem, guard_skipped=guard_skipped)
    assert bool((o["p"] == P).all())
    return dict(p=P, g=o["g"], m=M, v=V, mem=o["mem"])


def check(nat, case, hp, zero_grad=1, ema_decay=None, guard_skipped=False, **kw):
    """One exact launch against the oracle, whole buffers."""
    A = case.A
    before = {k: b.host() for k, b in case.buffers().items()}
    b64 = (*A.host64(), case.V.inner.cpu().double())
    e64 = case.E.inner.cpu().double()
    if ema_decay is not None:
        kw = dict(kw, ema=case.E.ptr, ema_one_minus_decay=ex.omd_of(ema_decay))
    launch(nat, case, hp, zero_grad, **kw)
    o = expected(case, b64, hp, zero_grad, guard_skipped)
    for name, buf, key in (("p", A.p, "p"), ("buf", A.buf, "m"), ("v", case.V, "v"), ("g", A.g, "g")):
        same_bits(buf.host(), buf.expect(before[name], f32_of(o[key])), name)
    for q, b in case.mem.items():
        same_bits(b.host(), b.expect(before[f"bf16 copy {q}"], ux.bf16_of(o["mem"][q])),
                  f"bf16 copy {q}")
    same_bits(case.part.host(), before["lamb_partial"], "the partial table is read only")
    if guard_skipped:
        same_bits(case.trust.host(), before["lamb_trust"], "skipped step: the stored ratios stay")
    else:
        assert bool((o["p"] != b64[0])[case.mask].any())
        same_bits(case.trust.host(), case.trust.expect(before["lamb_trust"],
                                                       torch.tensor(case.TRUST)), "stored ratios")
    if ema_decay is None or guard_skipped:
        same_bits(case.E.host(), before["ema"], "ema: not this launch's")
    else:
        want = torch.where(case.mask, ex.ema_ref(e64, o["p"], ex.omd_of(ema_decay), exact=True), e64)
        same_bits(case.E.host(), case.E.expect(before["ema"], f32_of(want)), "ema")
    return o


@pytest.mark.parametrize("ema", [0, 1], ids=["noema", "ema"])
@pytest.mark.parametrize("guard", [0, 1], ids=["plain", "guard"])
def test_lamb_update_exact(native_ext, guard, ema):
    """All four LAMB instantiations: p, m, v, the EMA (decay 0.75) and every bf16 copy bit for bit
    with ratios 2^-1, 1 and 2 on different tensors; a tensor that is not adapted ignores its
    partials, one with wn == 0 takes 1; the stored ratios are the hand-made ones; the guard at
    c == 1 leaves the same bits."""
    case = Case(native_ext, True)
    kw, keep = ex.variant(case, 0, guard)
    check(native_ext, case, EXACT_HP, ema_decay=0.75 if ema else None, **kw)
    case.pad_channels_are_zero()
    if guard:
        assert ux.f32_bits(1.0) == int(keep[-1][1].inner.cpu()[1])


def test_zero_grad_0_keeps_the_gradient(native_ext):
    case = Case(native_ext, True, seed=172)
    o = check(native_ext, case, EXACT_HP, zero_grad=0)
    assert bool((o["g"] != 0).any())


@pytest.mark.parametrize("guard", [0, 1], ids=["plain", "guard"])
def test_skip_word_leaves_everything(native_ext, guard):
    case = Case(native_ext, True, seed=173)
    kw, keep = ex.variant(case, 0, guard)
    skip = torch.ones(1, dtype=torch.int32, device=DEV)
    before = {k: b.host() for k, b in case.buffers().items()}
    launch(native_ext, case, EXACT_HP, skip=skip.data_ptr(), ema=case.E.ptr,
           ema_one_minus_decay=0.25, **kw)
    for k, b in case.buffers().items():
        same_bits(b.host(), before[k], f"skip word set: {k}")


@pytest.mark.parametrize("zero_grad", [0, 1])
def test_guard_skipped_step_clears_g_only_and_keeps_the_ratios(native_ext, zero_grad):
    case = Case(native_ext, True, seed=174)
    ckw, bufs = ex.guard_kw([1.0, float("inf"), 1.0], 2.0, 2 | 4)
    check(native_ext, case, EXACT_HP, zero_grad=zero_grad, ema_decay=0.75, guard_skipped=True, **ckw)
    assert int(bufs[1].inner.cpu()[2]) == 6   # counted


def test_table_index_clamps_to_the_last_entries(native_ext):
    case = Case(native_ext, True, seed=175)
    check(native_ext, case, EXACT_HP, step=9, n_lr=4, n_bias=3)


def test_refused_argument_combinations(native_ext):
    case = Case(native_ext, True, seed=176)
    before = {k: b.host() for k, b in case.buffers().items()}
    lkw, keep = ex.lars_unit(len(case.items))
    with pytest.raises(RuntimeError):
        launch(native_ext, case, EXACT_HP, **lkw)
    h = dict(ux.EXACT, nesterov=0)
    with pytest.raises(RuntimeError):   # LambArgs without AdamArgs
        ux.launch(native_ext, case.items, case.rows, case.A, h, **case.lamb_kw())
    for missing in ("lamb_tensors", "lamb_partial", "lamb_trust"):
        sched, bias = gx.tables(EXACT_HP)
        with pytest.raises(RuntimeError):
            ux.launch(native_ext, case.items, case.rows, case.A, h,
                      **gx.adam_kw(case, EXACT_HP, sched, bias), **dict(case.lamb_kw(), **{missing: 0}))
    for k, b in case.buffers().items():
        same_bits(b.host(), before[k], f"refused launch: {k}")


# --------------------------------------------------------- both kernels chained, bound mode
def _lamb_rig(seed=3, **kw):
    """tests/test_gpu_lars.py _kernel_params under LAMB: randn gradients (one 2-D tensor's stay
    zero), a history in m and v, the table entry of t = 3."""
    from ddp_amd.optim import LAMB
    ps, specs = gl._kernel_params()
    opt = LAMB(ps, grad_scale=0.5, **kw)
    for sp in specs:
        sp.maybe_pack()
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    opt.momentum_buffer.copy_(0.1 * torch.randn(opt.arena.total, device=DEV, generator=g))
    opt.second_moment.copy_(0.02 * torch.rand(opt.arena.total, device=DEV, generator=g) + 1e-6)
    gl._set_grads(ps, gl._grads(ps, seed + 2))
    opt.set_lr_step(2)
    torch.cuda.synchronize()
    return ps, specs, opt


def _views(opt, i):
    a = opt.arena
    return [a.shaped(t, i).detach().cpu().double().reshape(-1)
            for t in (a.data, a.grad, opt.momentum_buffer, opt.second_moment)]


def test_chained_kernels_bound(native_ext):
    ps, specs, opt = _lamb_rig()
    kinds = set(int(k) for k in opt._work_table()[0][:, 0].tolist())
    assert kinds == {0, 1, 2}
    assert [opt.arena.numels[i] for i in gl.ADAPTED] == [1728, 41472, 330]
    n = len(ps)
    state0 = [_views(opt, i) for i in range(n)]
    opt.step(zero_grad=True)
    torch.cuda.synchronize()
    a1, a2 = opt.bias_at(2)
    hp = ao.hyper(1e-3, 1e-2, 0.5, 0.9, 0.999, 1e-8, a1, a2)
    stored = opt.trust_ratios().cpu()
    for i in range(n):
        p, g, m, v = state0[i]
        adapted = ps[i].dim() > 1
        r = lo.direction(p, g, m, v, hp)[0]
        T = lo.lamb_abs(p, g, m, v, hp)
        want_t = lo.trust_of(lo.sum_sq(p), lo.sum_sq(r), adapted)
        got_t = float(stored[i])
        if adapted:
            rtol = lo.trust_rtol(r, T["T_r"], FP32_EPS)
            print(f"parameter {i}: trust {got_t!r} rel err {abs(got_t - want_t) / want_t:.3e} "
                  f"bound {rtol:.3e}")
            assert abs(got_t - want_t) <= rtol * want_t and got_t != 1.0, i
        else:
            assert got_t == 1.0, i
        want = lo.lamb_ref(p, g, m, v, hp, trust=got_t)   # the ratio the device stored
        bd = lo.bounds(T, FP32_EPS, hp["lr"] * got_t)
        got = _views(opt, i)
        for name, gt, w in (("p", got[0], want[0]), ("m", got[2], want[1]), ("v", got[3], want[2])):
            worst = assert_within(gt.float(), w, bd[name], what=f"parameter {i}: {name}")
        assert not bool(got[1].any()), f"parameter {i}: gradient not cleared"
    # bf16 operand copies == bf16(new master), exactly
    c0, c1 = ps[0].detach(), ps[4].detach()
    wc0 = specs[0].wc.view(64, 3, 3, 8).float()
    assert torch.equal(wc0[..., :3], c0.permute(0, 2, 3, 1).to(torch.bfloat16).float())
    assert float(wc0[..., 3:].abs().max()) == 0.0
    assert torch.equal(specs[1].wc.view(72, 3, 3, 64).float(),
                       c1.permute(0, 2, 3, 1).to(torch.bfloat16).float())


def test_two_runs_are_bit_identical(native_ext):
    pa, sa, oa = _lamb_rig(5, max_grad_norm=1.0)
    pb, sb, ob = _lamb_rig(5, max_grad_norm=1.0)
    oa.set_ema(0.9)
    ob.set_ema(0.9)
    oa.step(zero_grad=True)
    ob.step(zero_grad=True)
    torch.cuda.synchronize()
    assert float(oa.clip_coef()) < 1.0
    for x, y in ((oa.arena.data, ob.arena.data), (oa.momentum_buffer, ob.momentum_buffer),
                 (oa.second_moment, ob.second_moment), (oa.ema, ob.ema),
                 (oa.trust_ratios(), ob.trust_ratios())):
        assert torch.equal(x, y)


def test_per_range_launches_equal_the_whole_launch_and_follow_the_cpu_class(native_ext):
    """``step(params=...)`` over a partition -- what the pipelined step issues per bucket -- leaves
    the bits of one whole launch, ratios included. The CPU class on the same state takes its sums
    in fp64, so its ratios differ from the device's by the chain's roundings: each side is within
    lamb_oracle's bounds of the fp64 rule, so the two are within their sum of each other."""
    from ddp_amd.optim import LAMB
    pa, sa, oa = _lamb_rig(7)
    pb, sb, ob = _lamb_rig(7)
    n = len(pa)
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in pa]
    copt = LAMB(cpu, grad_scale=0.5)
    for i, c in enumerate(cpu):
        c.grad = oa.arena.shaped(oa.arena.grad, i).detach().cpu().clone()
        copt.state[c] = {"step": torch.tensor(2.0),
                         "exp_avg": oa.arena.shaped(oa.momentum_buffer, i).cpu().clone(),
                         "exp_avg_sq": oa.arena.shaped(oa.second_moment, i).cpu().clone()}
    copt.set_lr_step(2)
    state0 = [_views(oa, i) for i in range(n)]
    oa.step(zero_grad=True)
    for rng in ((0, 3), (3, 5), (5, n)):
        ob.step(zero_grad=True, params=rng, lr_advance=(rng[1] == n))
    copt.step()
    torch.cuda.synchronize()
    assert oa.lr_step == ob.lr_step == copt.lr_step == 3 == ob.lr_step_device()
    for what, x, y in (("p", oa.arena.data, ob.arena.data), ("m", oa.momentum_buffer, ob.momentum_buffer),
                       ("v", oa.second_moment, ob.second_moment), ("g", oa.arena.grad, ob.arena.grad),
                       ("trust", oa.trust_ratios(), ob.trust_ratios())):
        same_bits(x.cpu(), y.cpu(), what, guard=0)
    for s, t in zip(sa, sb):
        same_bits(s.wc.cpu().reshape(-1), t.wc.cpu().reshape(-1), "Wc", guard=0)
    a1, a2 = oa.bias_at(2)
    hp = ao.hyper(1e-3, 1e-2, 0.5, 0.9, 0.999, 1e-8, a1, a2)
    for i in range(n):
        p, g, m, v = state0[i]
        T = lo.lamb_abs(p, g, m, v, hp)
        r = lo.direction(p, g, m, v, hp)[0]
        tg, tc = float(oa.trust_ratios()[i]), float(copt.trust_ratios()[i])
        rtol = lo.trust_rtol(r, T["T_r"], FP32_EPS)
        assert abs(tg - tc) <= 2 * rtol * tc, i
        bd = lo.bounds(T, FP32_EPS, hp["lr"] * max(tg, tc))["p"]
        drift = hp["lr"] * abs(tg - tc) * r.abs()   # the two ratios apart
        assert_within(oa.arena.shaped(oa.arena.data, i).detach().cpu().reshape(-1),
                      cpu[i].detach().double().reshape(-1), 2 * bd + drift,
                      what=f"parameter {i}: GPU against the CPU class")


def test_state_snapshot_carries_the_ratios_inputs(native_ext):
    """m, v, the step and the EMA come back; then the same gradient gives the same ratios."""
    pa, sa, oa = _lamb_rig(9)
    oa.set_ema(0.9)
    p0, g0 = oa.arena.data.clone(), oa.arena.grad.clone()
    want = [t.clone() for t in (oa.momentum_buffer, oa.second_moment, oa.ema)]
    snap = oa.state_snapshot()
    oa.step()
    torch.cuda.synchronize()
    first = oa.trust_ratios().clone()
    p1 = oa.arena.data.clone()
    assert oa.lr_step == 3 and not torch.equal(oa.second_moment, want[1])
    oa.restore_state(snap)
    oa.arena.data.copy_(p0)
    oa.arena.grad.copy_(g0)
    assert oa.lr_step == 2 == oa.lr_step_device()
    for t, w in zip((oa.momentum_buffer, oa.second_moment, oa.ema), want):
        assert torch.equal(t, w)
    oa.trust_ratios().fill_(7.0)
    oa.step()
    torch.cuda.synchronize()
    assert torch.equal(oa.trust_ratios(), first) and torch.equal(oa.arena.data, p1)
