"""The weight EMA of the fused update launch (csrc/kernels/optim.hip, the EMA instantiations of
sgd_pack_kernel; api.h EmaArgs) against a CPU oracle, element for element and bit for bit, with
the guard-band convention of tests/test_gpu_update_exact.py (whose helpers are used here): 64
elements of a NaN pattern around p, g, buf, ema and every bf16 copy, WHOLE buffers compared.

Oracle: tests/update_oracle.py's step, then for every element whose master an item of kind 0-3
updates

    e' = e + omd * (p_new - e)         in fp64, omd = float32(1 - decay)

Exact mode: the update_exact hyper-parameters, decay 0.75 (omd = 2**-2), p / g / buf / ema integers
in [-64, 64], two steps. The oracle asserts that p_new - e and e' are fp32 numbers, so neither
the subtraction nor the fma rounds and ema must equal the oracle.

Bound mode: randn inputs, the project's hyper-parameters, decay 0.999, one step on a non-zero
momentum and EMA history. The roundings behind e': the R_p (4, 5 with nesterov) of p_new, the
subtraction and the fma. With T_p the oracle's pass over the magnitudes behind p_new,
    |fl(p_new) - p_new|            <= R_p eps T_p
    |fl(p_new - e) - (p_new - e)|  <= that + eps (T_p + |e|)
    |fl(e') - e'|                  <= omd (R_p eps T_p + eps (T_p + |e|)) + eps (|e| + omd (T_p + |e|))
                                   <= (R_p + 2) eps T,     T = |e| + omd (T_p + |e|)
(the lerp on the magnitudes, the subtraction taken as a sum). p, buf, g and the bf16 copies must
be bitwise what the same launch without EmaArgs writes: the EMA does not perturb the update.
"""
import numpy as np
import pytest
import torch

import test_gpu_update_exact as ux
import update_oracle as uo
from exactness import FP32_EPS, assert_within, int_tensor

pytestmark = pytest.mark.gpu

DEV = "cuda"
Buf, same_bits, f32_of = ux.Buf, ux.same_bits, ux.f32_of


def omd_of(decay):
    return float(np.float32(1.0 - decay))


def ema_ref(e, p_new, omd, exact=False):
    """fp64 lerp; ``exact``: assert that no fp32 operation behind it rounds."""
    d = p_new - e
    r = e + omd * d
    if exact:
        assert bool(uo.is_f32(d).all()), "ema_ref exact mode: p_new - e is not an fp32 number"
        assert bool(uo.is_f32(r).all()), "ema_ref exact mode: e + omd (p_new - e) is not an fp32 number"
    return r


def updated_mask(items, rows, n):
    """Elements whose master a launch of ``items`` updates: the oracle on marker data (p = 0,
    g = 1, lr = 1: the new p is -1 exactly there)."""
    z = torch.zeros(n, dtype=torch.float64)
    h = dict(lr=1.0, momentum=0.0, wd=0.0, grad_scale=1.0, nesterov=0)
    mem = {}
    for r in rows:
        for q in (6, 7):
            if int(r[q]):
                mem[int(r[q])] = np.zeros(int(r[1]) * int(r[3]) * int(r[4]) * int(r[5]), np.uint16)
    o = uo.run_items(items, rows, z, z + 1.0, z, h, mem=mem, shadow=np.zeros(n, np.uint16),
                     slot=torch.zeros(n, dtype=torch.float64))
    return o["p"] != 0


# ------------------------------------------------------------------------------------ the table
def ema_table():
    """The smallest shapes that reach every path of the EMA. Returns items, descriptor rows
    (entries 6 / 7 hold the bf16 element counts until the case allocates them), arena size.
      kind 0: 1 element; 7 elements from an offset with off & 3 == 1 (the scalar path only);
              8192 + 4 elements (two chunks, float4 path)
      kind 2: a [K][R][S][C] conv 64 x 3 x 3 x 64 (36 864 elements: five chunks, the last one
              half) and a 1x1 conv 64 -> 64
      kind 1: the channel-padded input layer, K 64, Cr 3 of C 8, 3x3, stored [K][R][S][Cr]
              (ema holds K * Cr * 9 values; the Wc pad channels get +0)
      kind 1: a [K][C][R][S] master with Wt, K 40, C 48, 3x3: 32 x 32 tiles cut at both edges"""
    rows, items, off = [], [], 64

    def conv(K, Cr, C, R, krsc, wt):
        nonlocal off
        rows.append([off, K, Cr, C, R, R, K * R * R * C, C * R * R * K if wt else 0, krsc, 0, 0, 0])
        off += (K * Cr * R * R + 63) // 64 * 64 + 64
        return len(rows) - 1

    d0 = conv(64, 64, 64, 3, 1, False)
    d1 = conv(64, 64, 64, 1, 0, False)
    d2 = conv(64, 3, 8, 3, 1, False)
    d3 = conv(40, 48, 48, 3, 0, True)
    n0 = 64 * 64 * 9
    items += [[2, s, min(8192, n0 - s), d0] for s in range(0, n0, 8192)]
    items += [[2, 0, 4096, d1]]
    items += uo.tile_items(d2, rows[d2]) + uo.tile_items(d3, rows[d3])
    items.append([0, off, 1, 0])
    off += 8
    assert (off + 1) & 3 == 1
    items.append([0, off + 1, 7, 0])
    off += 16
    items += [[0, off, 8192, 0], [0, off + 8192, 4, 0]]
    off += 8192 + 4 + 60
    order = np.random.RandomState(5).permutation(len(items))
    return [items[i] for i in order], rows, off + 64


class Case:
    """ema_table() on the device: arena, EMA, bf16 copies (prefilled, pad channels poisoned)."""

    def __init__(self, nat, exact, seed=61):
        self.items, self.rows, n = ema_table()
        assert {it[0] for it in self.items} == {0, 1, 2}
        self.exact = exact
        self.A = ux.Arena(n, seed, exact)
        self.E = Buf(n, fill=self.A._draw(seed + 50))
        self.mem = {}
        for r in self.rows:
            wc = Buf(r[6], torch.bfloat16)
            wt = Buf(r[7], torch.bfloat16) if r[7] else None
            r[6], r[7] = wc.ptr, wt.ptr if wt else 0
            ux.prefill(nat, self.A, r, wc, wt)
            self.mem[wc.ptr] = wc
            if wt:
                self.mem[wt.ptr] = wt
        self.mask = updated_mask(self.items, self.rows, n)
        # exactly the masters: K * Cr * R * S per conv, the plain chunks, nothing in between
        want = sum(r[1] * r[2] * r[4] * r[5] for r in self.rows) + 1 + 7 + 8192 + 4
        assert int(self.mask.sum()) == want

    def buffers(self):
        return dict(p=self.A.p, g=self.A.g, buf=self.A.buf, ema=self.E,
                    **{f"bf16 copy {k}": b for k, b in self.mem.items()})

    def pad_channels_are_zero(self):
        r = self.rows[2]
        K, Cr, C, R = r[1], r[2], r[3], r[4]
        wc = self.mem[r[6]].np_bits().reshape(K, R, R, C)
        assert (wc[..., Cr:] == 0).all()


def check_ema_launch(nat, case, h, steps, decay, **kw):
    """``steps`` launches with EmaArgs: p, g, buf and every bf16 copy through
    test_gpu_update_exact.check_launch, ema against ``ema_ref`` over the oracle's new p."""
    omd = omd_of(decay)
    A, E = case.A, case.E
    for step in range(steps):
        if step:
            A.new_grad(step)
        eb, e64 = E.host(), E.inner.cpu().double()
        p64 = A.host64()
        o = ux.check_launch(nat, case.items, case.rows, A, h, 1, mem=case.mem, ema=E.ptr,
                            ema_one_minus_decay=omd, **kw)
        if kw.get("guard_skipped"):
            same_bits(E.host(), eb, f"step {step}: ema after a skipped step")
            continue
        if case.exact:
            want = torch.where(case.mask, ema_ref(e64, o["p"], omd, exact=True), e64)
            same_bits(E.host(), E.expect(eb, f32_of(want)), f"step {step}: ema")
            assert bool((want != e64)[case.mask].any())
        else:
            want = torch.where(case.mask, ema_ref(e64, o["p"], omd), e64)
            t = uo.run_items(case.items, case.rows, *p64, h, abs_pass=True)
            T = e64.abs() + omd * (t["p"] + e64.abs())
            bound = torch.where(case.mask, (ux.r_p(h["nesterov"]) + 2) * FP32_EPS * T, 0.0)
            worst = assert_within(E.inner.cpu(), want, bound, what=f"step {step}: ema")
            print(f"bound mode: worst |err|/bound ema {worst:.3f}")
            got = E.host()
            same_bits(got, E.expect(eb, got[ux.GUARD:ux.GUARD + E.n]), "ema guards")
    return o


# ------------------------------------------------------------------- LARS and guard arguments
def lars_unit(n_items):
    """LARS arguments that give every item the trust ratio 1.0: one parameter, not adapted."""
    side = torch.tensor([[0, int(i == 0)] for i in range(n_items)], dtype=torch.int32, device=DEV)
    tensors = torch.tensor([[0, 1, 0, 0]], dtype=torch.int32, device=DEV)
    partial = torch.ones(1, 2, dtype=torch.float32, device=DEV)
    trust = torch.full((1,), 7.0, dtype=torch.float32, device=DEV)
    kw = dict(lars_side=side.data_ptr(), lars_tensors=tensors.data_ptr(),
              lars_partial=partial.data_ptr(), lars_trust=trust.data_ptr(), lars_eta=0.5,
              lars_eps=0.0)
    return kw, (side, tensors, partial, trust)


def guard_kw(partials, max_norm, flags):
    part, stats = ux.guard_buffers(partials)
    return dict(clip_partial=part.ptr, clip_chunks=len(partials), clip_max_norm=max_norm,
                clip_eps=0.0, clip_flags=flags, clip_stats=stats.ptr), (part, stats)


def variant(case, lars, guard):
    """Keywords of the instantiation <lars, guard, EMA> that must reproduce the plain update:
    trust ratio 1 (LARS), c == 1 (guard: norm 4 below max_norm 8)."""
    kw, keep = {}, []
    if lars:
        k, t = lars_unit(len(case.items))
        kw.update(k)
        keep.append(t)
    if guard:
        k, t = guard_kw([4.0, 0.0, 12.0], 8.0, 1 | 2 | 4)
        kw.update(k)
        keep.append(t)
    return kw, keep


# ------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("guard", [0, 1], ids=["plain", "guard"])
@pytest.mark.parametrize("lars", [0, 1], ids=["sgd", "lars"])
def test_ema_exact(native_ext, lars, guard):
    """All four EMA instantiations, two exact steps; with LARS at ratio 1 and the guard at c == 1
    the bits are the plain EMA's (the same oracle)."""
    case = Case(native_ext, True)
    kw, keep = variant(case, lars, guard)
    h = dict(ux.EXACT, nesterov=0, zero_grad=1)
    check_ema_launch(native_ext, case, h, 2, 0.75, **kw)
    case.pad_channels_are_zero()
    if lars:
        assert float(keep[0][3][0]) == 1.0   # the ratio was stored
    if guard:
        assert ux.f32_bits(1.0) == int(keep[-1][1].inner.cpu()[1])


@pytest.mark.parametrize("nesterov,momentum", [(1, 0.5), (0, 0.0)])
def test_ema_exact_branches(native_ext, nesterov, momentum):
    case = Case(native_ext, True, seed=62)
    h = dict(ux.EXACT, momentum=momentum, nesterov=nesterov, zero_grad=0)
    check_ema_launch(native_ext, case, h, 2, 0.75)


@pytest.mark.parametrize("lars", [0, 1], ids=["sgd", "lars"])
def test_ema_follows_the_clipped_update(native_ext, lars):
    """Partials {4, 0, 12}: norm 4, c = 2 / 4 = 0.5, the update runs with grad_scale 2**-2 and
    the EMA takes that p_new."""
    case = Case(native_ext, True, seed=63)
    kw, keep = ({}, None)
    if lars:
        kw, keep = lars_unit(len(case.items))
    ckw, bufs = guard_kw([4.0, 0.0, 12.0], 2.0, 1 | 2 | 4)
    h = dict(ux.EXACT, nesterov=0, zero_grad=1)
    check_ema_launch(native_ext, case, h, 1, 0.75, ohyper=dict(h, grad_scale=2.0 ** -2),
                     **kw, **ckw)
    assert int(bufs[1].inner.cpu()[1]) == ux.f32_bits(0.5)


@pytest.mark.parametrize("lars", [0, 1], ids=["sgd", "lars"])
def test_guard_skipped_step_leaves_the_ema(native_ext, lars):
    case = Case(native_ext, True, seed=64)
    kw, keep = ({}, None)
    if lars:
        kw, keep = lars_unit(len(case.items))
    ckw, bufs = guard_kw([1.0, float("inf"), 1.0], 2.0, 2 | 4)
    h = dict(ux.EXACT, nesterov=0, zero_grad=1)
    check_ema_launch(native_ext, case, h, 1, 0.75, guard_skipped=True, **kw, **ckw)
    assert int(bufs[1].inner.cpu()[2]) == 6   # counted


@pytest.mark.parametrize("guard", [0, 1], ids=["plain", "guard"])
@pytest.mark.parametrize("lars", [0, 1], ids=["sgd", "lars"])
def test_skip_word_leaves_everything(native_ext, lars, guard):
    case = Case(native_ext, True, seed=65)
    kw, keep = variant(case, lars, guard)
    skip = torch.ones(1, dtype=torch.int32, device=DEV)
    before = {k: b.host() for k, b in case.buffers().items()}
    ux.launch(native_ext, case.items, case.rows, case.A, dict(ux.EXACT, nesterov=0, zero_grad=1),
              skip=skip.data_ptr(), ema=case.E.ptr, ema_one_minus_decay=0.25, **kw)
    for k, b in case.buffers().items():
        same_bits(b.host(), before[k], f"skip word set: {k}")


@pytest.mark.parametrize("nesterov", [0, 1])
def test_ema_bound_and_update_unperturbed(native_ext, nesterov):
    h = dict(ux.PROJECT, nesterov=nesterov, zero_grad=1)
    plain, case = Case(native_ext, False, seed=66), Case(native_ext, False, seed=66)
    for a, b in zip(plain.buffers().values(), case.buffers().values()):
        same_bits(a.host(), b.host(), "the two cases start from the same bits")
    eb = plain.E.host()
    ux.launch(native_ext, plain.items, plain.rows, plain.A, h)
    check_ema_launch(native_ext, case, h, 1, 0.999)
    for (k, a), b in zip(plain.buffers().items(), case.buffers().values()):
        if k != "ema":
            same_bits(a.host(), b.host(), f"{k}: with EmaArgs against without")
    same_bits(plain.E.host(), eb, "ema without EmaArgs")


# ------------------------------------------------------------------- through the Python classes
def _int_like(t, seed):
    return int_tensor(tuple(t.shape), -64, 64, seed).to(t.device)


def _rig(cls, seed):
    """Two convs (the channel-padded input layer: tile items; a [K][R][S][C] one: item 2), their
    BatchNorm vectors and a two-chunk vector, all integers; EMA on with decay 0.75 and an integer
    history of its own."""
    from ddp_amd.ops.layers import ConvBNActSpec
    torch.manual_seed(seed)
    c0 = torch.nn.Conv2d(3, 64, 3, padding=1).to(DEV)
    b0 = torch.nn.BatchNorm2d(64).to(DEV)
    c1 = torch.nn.Conv2d(64, 48, 3, padding=1).to(DEV)
    extra = torch.nn.Parameter(torch.zeros(8192 + 5, device=DEV))
    specs = [ConvBNActSpec(c0, b0, cin_pad=8), ConvBNActSpec(c1, None)]
    params = list(c0.parameters()) + list(b0.parameters()) + list(c1.parameters()) + [extra]
    kw = dict(trust_coefficient=2.0 ** -3, eps=0.0) if cls.__name__ == "LARS" else {}
    opt = cls(params, momentum=ux.EXACT["momentum"], weight_decay=ux.EXACT["wd"],
              lr=ux.EXACT["lr"], grad_scale=ux.EXACT["grad_scale"], **kw)
    with torch.no_grad():
        for i, p in enumerate(params):
            p.copy_(_int_like(p, 500 + i))
    for sp in specs:
        sp.maybe_pack()
    opt.set_ema(0.75)
    opt.load_ema_state({i: _int_like(p, 600 + i).cpu() for i, p in enumerate(params)})
    for i, p in enumerate(params):
        p.grad.copy_(_int_like(p, 700 + i))
    torch.cuda.synchronize()
    return params, specs, opt


@pytest.mark.parametrize("cls_name", ["FusedSGD", "LARS"])
def test_per_range_launches_equal_the_whole_launch(native_ext, cls_name):
    """``step(params=...)`` over a 3-way partition of the parameters -- what the pipelined step
    issues per bucket -- leaves the bits of one whole launch: p, buf, ema, the operand copies."""
    import ddp_amd.optim as optim
    cls = getattr(optim, cls_name)
    pa, sa, oa = _rig(cls, 1)
    pb, sb, ob = _rig(cls, 1)
    e0 = oa.ema.clone()
    oa.step(zero_grad=True)
    n = len(pb)
    for rng in ((0, 2), (2, 5), (5, n)):
        ob.step(zero_grad=True, params=rng)
    torch.cuda.synchronize()
    assert not torch.equal(oa.ema, e0)
    for what, x, y in (("p", oa.arena.data, ob.arena.data), ("ema", oa.ema, ob.ema),
                       ("buf", oa.momentum_buffer, ob.momentum_buffer),
                       ("g", oa.arena.grad, ob.arena.grad)):
        same_bits(x.cpu(), y.cpu(), what, guard=0)
    for s, t in zip(sa, sb):
        same_bits(s.wc.cpu().reshape(-1), t.wc.cpu().reshape(-1), "Wc", guard=0)
    # and the whole launch is the formula: per parameter, against ema_ref over the new masters
    if cls_name == "FusedSGD":
        for i, p in enumerate(pa):
            e = _int_like(p, 600 + i).cpu().double()
            want = ema_ref(e, p.detach().cpu().double(), 0.25, exact=True)
            same_bits(oa.ema_state()[i], f32_of(want), f"ema of parameter {i}", guard=0)


def _copies(plan):
    return [t.clone() for sp in plan for t in (sp.wc, getattr(sp, "wt", None)) if t is not None]


def test_swap_ema_twice_restores_every_bit_vgg11(native_ext):
    """VGG-11: two swaps restore masters, momentum and every bf16 operand copy (Wc and Wt, padded
    channels included). After one swap the model runs on the average: its masters and operand
    copies are those of a second model loaded from ``ema_state()``, and ``forward_metrics`` on a
    64-image batch agrees with that model's (the release build's batch statistics use float
    atomics, so the metrics are compared to the bound of test_gpu_model's
    test_fused_eval_metrics_match, 5e-3 relative and one hit, and the weights bitwise)."""
    from ddp_amd.models import VGG11
    from ddp_amd.optim import FusedSGD
    torch.manual_seed(5)
    m = VGG11().cuda()
    opt = FusedSGD(m.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
    plan = m.fused_plan()
    for sp in plan:
        sp._packed_version = None
        sp.maybe_pack()
    opt.momentum_buffer.normal_()
    opt.set_ema(0.9)
    g = torch.Generator(device="cuda").manual_seed(6)
    for i in range(len(opt.arena.params)):   # an average of its own: 0.9 w + noise
        e = opt._ema_view(i)
        e.mul_(0.9).add_(0.01 * torch.randn(e.shape, device="cuda", generator=g))
    torch.cuda.synchronize()
    snap = (opt.arena.data.clone(), opt.momentum_buffer.clone(), opt.ema.clone(), _copies(plan))
    ptrs = (opt.arena.data.data_ptr(), opt.ema.data_ptr())
    x = torch.randn(64, 3, 32, 32, device="cuda")
    y = torch.randint(0, 10, (64,), device="cuda")

    def metrics(model):
        la = torch.zeros((), device="cuda")
        hits = torch.zeros((), dtype=torch.int32, device="cuda")
        model.eval()
        model.forward_metrics(x, y, la, hits)
        torch.cuda.synchronize()
        model.train()
        return float(la), int(hits)

    raw = metrics(m)
    m2 = VGG11().cuda()
    average = opt.ema_state(m)
    missing = m2.load_state_dict({k: v.cuda() for k, v in average.items()}, strict=False)
    assert not missing.unexpected_keys
    assert not [k for k in missing.missing_keys if k in dict(m2.named_parameters())]
    opt.swap_ema()
    torch.cuda.synchronize()
    same_bits(opt.arena.data.cpu(), snap[2].cpu(), "masters after one swap", guard=0)
    same_bits(opt.ema.cpu(), snap[0].cpu(), "ema after one swap", guard=0)
    for k, p in m.named_parameters():   # the model now holds the average
        assert average[k].shape == p.shape
        same_bits(p.detach().cpu().contiguous(), dict(m2.named_parameters())[k].detach().cpu(),
                  f"{k}: swapped-in master", guard=0)
    plan2 = m2.fused_plan()
    for sp in plan2:
        sp._packed_version = None
        sp.maybe_pack()
    torch.cuda.synchronize()
    for j, (a, b) in enumerate(zip(_copies(plan), _copies(plan2))):
        same_bits(a.cpu().reshape(-1), b.cpu().reshape(-1), f"operand copy {j} after one swap",
                  guard=0)
    la, ha = metrics(m)
    lb, hb = metrics(m2)
    assert abs(la - lb) < 5e-3 * max(1.0, abs(lb)) and abs(ha - hb) <= 1
    assert (la, ha) != raw   # the average is not the raw weights
    opt.swap_ema()
    torch.cuda.synchronize()
    assert (opt.arena.data.data_ptr(), opt.ema.data_ptr()) == ptrs
    for what, got, want in (("masters", opt.arena.data, snap[0]), ("ema", opt.ema, snap[2]),
                            ("momentum", opt.momentum_buffer, snap[1])):
        same_bits(got.cpu(), want.cpu(), f"{what} after two swaps", guard=0)
    for j, (a, b) in enumerate(zip(_copies(plan), snap[3])):
        same_bits(a.cpu().reshape(-1), b.cpu().reshape(-1), f"operand copy {j} after two swaps",
                  guard=0)
