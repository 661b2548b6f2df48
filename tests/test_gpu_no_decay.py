"""The no-decay mask (optim/sgd.py ``no_decay``, --no-decay-1d) at the optimizer level on the GPU:
the work-item tables, eager and captured steps of FusedSGD, AdamW and LAMB against each other and
against their CPU twins, the VGG-11 training step (tests/no_decay_probe.py), the sharded update's
items and ``step_elements``. The raw launches: tests/test_gpu_no_decay_exact.py."""
import json
import os
import subprocess
import sys

import pytest
import torch

import adamw_oracle as ao
import decay_oracle as do
import lamb_oracle as lo
import test_gpu_lars as gl
import test_gpu_update_exact as ux
import update_oracle as uo
from exactness import FP32_EPS, assert_within, int_tensor

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
WD = 0.05
F = do.NO_DECAY


class _FlagOracle:
    run_items = staticmethod(do.run_items)

    def __getattr__(self, name):
        return getattr(uo, name)


@pytest.fixture(autouse=True)
def flag_oracle(monkeypatch):
    monkeypatch.setattr(ux, "uo", _FlagOracle())


def _make(cls, no_decay, **kw):
    """tests/test_gpu_lars.py ``_kernel_params`` (item kinds 0, 1 and 2; five 1-D tensors)."""
    ps, specs = gl._kernel_params()
    opt = cls(ps, weight_decay=WD, no_decay=no_decay, **kw)
    for sp in specs:
        sp.maybe_pack()
    return ps, specs, opt


# ---------------------------------------------------------------------------------- the tables
def test_work_tables_with_the_mask_off_and_on(native_ext):
    from ddp_amd.optim import FusedSGD
    ps, specs, plain = _make(FusedSGD, None, lr=0.1)
    n = len(ps)
    ref = FusedSGD(ps, lr=0.1, weight_decay=WD)
    cut = 4
    for rng in (None, (0, cut), (cut, n)):
        a, b = plain._work_table(rng), ref._work_table(rng)
        assert a[1] == b[1] and torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
        assert a[0].dtype == b[0].dtype == torch.int32
    on = FusedSGD(ps, lr=0.1, weight_decay=WD, no_decay="1d")
    for rng in (None, (0, cut), (cut, n)):
        key = (tuple(rng) if rng else (0, n), frozenset(), frozenset())
        (ti, tn, td), (ri, rn, rd) = on._work_table(rng), ref._work_table(rng)
        owners = on._tables[key][2]
        assert tn == rn and torch.equal(td, rd) and owners == ref._tables[key][2]
        masked = torch.tensor([ps[i].dim() <= 1 for i in owners], device=DEV)
        assert bool(masked.any()) and not bool(masked.all())
        diff = ti - ri
        assert torch.equal(diff[:, 1:], torch.zeros_like(diff[:, 1:]))
        assert torch.equal(diff[:, 0], torch.where(masked, F, 0).to(torch.int32))
        assert torch.equal(ti[:, 0] & 0xff, ri[:, 0])
    # set_no_decay drops the cached tables; None brings the parent's back byte for byte
    on.set_no_decay(None)
    assert torch.equal(on._work_table()[0], ref._work_table()[0])


def test_chunk_tables_carry_the_flag_in_the_fourth_field(native_ext):
    from ddp_amd.optim import LAMB
    ps, specs, off = _make(LAMB, None, exclude_1d=False)
    ps2, specs2, on = _make(LAMB, "1d", exclude_1d=False)
    n = len(ps)
    t0, t1 = off._norm_table((0, n))[0].cpu(), on._norm_table((0, n))[0].cpu()
    assert torch.equal(t0[:, :3], t1[:, :3]) and not bool(t0[:, 3].any())
    starts = {on.arena.offsets[i] for i in range(n) if ps2[i].dim() <= 1}
    for row in t1.tolist():
        owner = max(i for i in range(n) if on.arena.offsets[i] <= row[0])
        assert row[3] == int(ps2[owner].dim() <= 1)
    assert starts <= {r[0] for r in t1.tolist()}


# ------------------------------------------------------- eager, captured and the CPU twin
def _grads(ps, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.randn(p.shape, device=DEV, generator=g) for p in ps]


def _state(opt, i):
    a = opt.arena
    arenas = [a.data, a.grad, opt.momentum_buffer] + \
        ([opt.second_moment] if hasattr(opt, "second_moment") else [])
    return [a.shaped(t, i).detach().cpu().double().reshape(-1) for t in arenas]


def _bound_vs_oracle(name, opt, i, st0, masked, lr):
    """(the fp64 rule's p', the kernel's bound on p') of parameter i for one step from ``st0``."""
    g = opt.param_groups[0]
    wd = 0.0 if masked else WD
    if name == "sgd":
        p, gr, buf = st0
        h = dict(lr=lr, momentum=g["momentum"], wd=wd, grad_scale=1.0, nesterov=0)
        want = uo.sgd_ref(p, gr, buf, **h)[0]
        return want, ux.r_p(0) * FP32_EPS * uo.sgd_abs(p, gr, buf, **h)[0]
    p, gr, m, v = st0
    a1, a2 = opt.bias_at(opt.lr_step - 1)
    hp = ao.hyper(lr, wd, 1.0, 0.9, 0.999, 1e-8, a1, a2)
    if name == "adamw":
        want = ao.adamw_ref(p, gr, m, v, hp)[0]
        return want, ao.bounds(ao.adamw_abs(p, gr, m, v, hp), FP32_EPS)["p"]
    t = float(opt.trust_ratios()[i])   # the ratio the device stored
    want = lo.lamb_ref(p, gr, m, v, hp, trust=t)[0]
    return want, lo.bounds(lo.lamb_abs(p, gr, m, v, hp), FP32_EPS, lr * t)["p"]


@pytest.mark.parametrize("name", ["sgd", "adamw", "lamb"])
def test_eager_captured_and_cpu_twin_agree(native_ext, name):
    """Three eager steps and three replays of a captured step (torch.cuda.graph, one stream: no
    parallel branches) agree bit for bit. Before every step the CPU twin takes the eager
    optimizer's state, and after it the two are within twice the kernel's one-step bound of each
    other: both are within that bound of the fp64 rule (LAMB: the CPU class takes its sums in fp64,
    so the two ratios' distance is added, as tests/test_gpu_lamb_exact.py does)."""
    from ddp_amd.optim import AdamW, FusedSGD, LAMB
    cls = dict(sgd=FusedSGD, adamw=AdamW, lamb=LAMB)[name]
    kw = dict(lr=0.05, momentum=0.9) if name == "sgd" else dict(lr=1e-3)
    pa, sa, oa = _make(cls, "1d", **kw)
    pb, sb, ob = _make(cls, "1d", **kw)
    n = len(pa)
    masked = [p.dim() <= 1 for p in pa]
    assert oa.no_decay_mask == masked
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in pa]
    copt = cls(cpu, weight_decay=WD, no_decay="1d", **kw)
    # warm up on a side stream (builds every device table), roll the state back, capture
    snap = [t.clone() for t in [oa.arena.data] + oa._state_arenas()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gl._set_grads(pa, _grads(pa, 49))
        oa.step(zero_grad=True, lr_advance=True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oa.step(zero_grad=True, lr_advance=True)
    for t, v in zip([oa.arena.data] + oa._state_arenas(), snap):
        t.copy_(v)
    oa.arena.grad.zero_()
    oa.set_lr_step(0)
    oa.repack()
    torch.cuda.synchronize()
    for k in range(3):
        gs = _grads(pa, 50 + k)
        gl._set_grads(pa, gs)
        gl._set_grads(pb, gs)
        st0 = [_state(ob, i) for i in range(n)]
        for i, c in enumerate(cpu):   # the twin starts every step from the device's state
            with torch.no_grad():
                c.copy_(pb[i].detach().cpu())
            c.grad = gs[i].cpu().clone()
            if name == "sgd":
                copt.state[c]["momentum_buffer"] = ob.arena.shaped(ob.momentum_buffer, i).cpu().clone()
            else:
                copt.state[c] = {"step": torch.tensor(float(k)),
                                 "exp_avg": ob.arena.shaped(ob.momentum_buffer, i).cpu().clone(),
                                 "exp_avg_sq": ob.arena.shaped(ob.second_moment, i).cpu().clone()}
        copt.set_lr_step(k)
        graph.replay()
        oa.count_step()
        ob.step(zero_grad=True, lr_advance=True)
        copt.step()
        torch.cuda.synchronize()
        gl._same(pa, sa, oa, pb, sb, ob)
        for x, y in zip(oa._state_arenas(), ob._state_arenas()):
            assert torch.equal(x, y)
        assert float(oa.arena.grad.abs().max()) == 0.0
        lr = kw["lr"]
        for i in range(n):
            want, bd = _bound_vs_oracle(name, ob, i, st0[i], masked[i], lr)
            got = pb[i].detach().cpu().reshape(-1)
            assert_within(got, want, bd, what=f"step {k} parameter {i}: GPU against the rule")
            drift = 0.0
            if name == "lamb":
                tg, tc = float(ob.trust_ratios()[i]), float(copt.trust_ratios()[i])
                p, gr, m, v = st0[i]
                a1, a2 = ob.bias_at(k)
                hp = ao.hyper(lr, 0.0 if masked[i] else WD, 1.0, 0.9, 0.999, 1e-8, a1, a2)
                r = lo.direction(p, gr, m, v, hp)[0]
                rtol = lo.trust_rtol(r, lo.lamb_abs(p, gr, m, v, hp)["T_r"], FP32_EPS)
                assert abs(tg - tc) <= 2 * rtol * tc, (k, i)
                drift = lr * abs(tg - tc) * r.abs()
            # the twin's own distance from the rule: AdamW's and LAMB's CPU paths take the
            # kernel's operations one for one (bd again); torch's SGD does not contract, 6
            # roundings behind p (wd p, + g, m buf, + d, lr buf, p -) against the kernel's 4
            twin = 6.0 / ux.r_p(0) if name == "sgd" else 1.0
            assert_within(got, cpu[i].detach().double().reshape(-1), (1 + twin) * bd + drift,
                          what=f"step {k} parameter {i}: GPU against the CPU twin")
    # the mask is in force: an unmasked optimizer on the same last step lands elsewhere on gamma
    assert masked[2] and bool((pa[2] != 1).any())


# ------------------------------------------------------------------------ VGG-11 training step
def test_train_step_keeps_sgd_in_the_backward_and_spares_the_gammas(native_ext):
    env = dict(os.environ, DDP_AMD_DETERMINISTIC="1")
    env.pop("DDP_AMD_SGD_IN_BWD", None)
    r = subprocess.run(["timeout", "-k", "10", "200", sys.executable,
                        os.path.join(REPO, "tests", "no_decay_probe.py")],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert res["gammas"] == 8
    assert res["opt_in_bwd"] is True and res["launch_only_opt_in_bwd"] is False
    assert res["in_bwd_equals_launch"] is True
    assert res["lr0_gammas_unchanged"] is True
    assert res["weights_equal"] is True and res["weights_moved"] is True
    # masked - unmasked = lr wd gamma on every gamma (= 1.0), to four half-ulps of values in
    # [1, 2): each side's last rounding, and the two of the decayed gradient scaled by lr
    assert res["gamma_shift_err"] <= 2.0 ** -22 < res["gamma_shift"] / 100


# ------------------------------------------------------------------------ the sharded update
@pytest.mark.parametrize("world", [2, 4])
def test_shard_items_carry_the_mask(native_ext, world):
    """``ShardedBf16Update.shard_items(j, r)`` for every rank of an emulated world: kind-3 pieces
    of masked tensors carry the flag, and the raw launch of each rank's table follows
    tests/decay_oracle.py bit for bit (exact mode, two steps), shadow and send slot included."""
    from ddp_amd.optim import FusedSGD
    from ddp_amd.parallel.zero import ShardedBf16Update
    torch.manual_seed(5)
    ps = [torch.nn.Parameter(torch.randn(*s, device=DEV)) for s in ((5, 12), (33,), (40, 10), (10,))]
    opt = FusedSGD(ps, lr=0.1, weight_decay=WD, no_decay="1d")
    a = opt.arena
    assert a.offsets == [0, 64, 128, 576] and a.total == 640

    class _Comm:
        rank, world = 0, 1
    upd = ShardedBf16Update(a, opt, _Comm(), [((0, 4), (0, a.total))], emulate_world=world)
    M = upd._plan[0]["M"]
    seen = set()
    for r in range(world):
        items = upd.shard_items(0, r)
        s0, s1 = upd.shard(0, r)
        for kind, off, cnt, slot in items:
            assert 0 <= off and off + cnt <= a.total and cnt % 4 == 0 and off % 4 == 0
            if kind & 0xff == 3:
                owner = max(i for i in range(4) if a.offsets[i] <= off)
                assert bool(kind & F) == (ps[owner].dim() <= 1) and s0 <= off < s1
                assert -1 <= slot and slot + cnt <= M
                seen.add((owner, bool(kind & F)))
            else:
                assert kind == 4
        A = ux.Arena(a.total, 300 + r)
        shadow = ux.Buf(a.total, torch.bfloat16)
        slot = ux.Buf(M, fill=torch.full((M,), -3.0))
        h = dict(ux.EXACT, nesterov=0, zero_grad=1)
        ux.check_launch(native_ext, items, [], A, h, 2, shadow=shadow, slot=slot)
    assert seen == {(0, False), (1, True), (2, False), (3, True)}


def test_step_elements_over_a_masked_and_an_unmasked_tensor(native_ext):
    """tests/test_gpu_update_exact.py test_step_elements_scalar_branch over two tensors: a masked
    vector of 8192 + 3 elements (padded to 8256) and a matrix behind it; the range starts off a
    multiple of 4 inside the vector and ends inside the matrix."""
    from ddp_amd.optim import FusedSGD
    E = ux.EXACT
    n0, n1 = 8192 + 3, 64 * 40
    vec = torch.nn.Parameter(int_tensor((n0,), -64, 64, 91).to(DEV))
    mat = torch.nn.Parameter(int_tensor((64, 40), -64, 64, 92).to(DEV))
    opt = FusedSGD([vec, mat], momentum=E["momentum"], weight_decay=E["wd"], lr=E["lr"],
                   grad_scale=E["grad_scale"], no_decay="1d")
    a = opt.arena
    o1 = a.offsets[1]
    assert o1 == 8256 and a.total == o1 + n1
    lo_, hi_ = 5, o1 + 1001
    items = opt._elem_table(lo_, hi_)[0].cpu().tolist()
    assert items == [[F, 5, 8192, 0], [F, 8197, o1 - 8197, 0], [0, o1, 1001, 0]]
    total = a.total
    p, buf = a.data.detach().cpu().double(), torch.zeros(total, dtype=torch.float64)
    for step in range(2):
        opt.zero_grad()
        vec.grad.copy_(int_tensor((n0,), -64, 64, 93 + step))
        mat.grad.copy_(int_tensor((64, 40), -64, 64, 95 + step))
        g = a.grad.detach().cpu().double()
        opt.step_elements(lo_, hi_, zero_grad=True)
        torch.cuda.synchronize()
        p, buf = p.clone(), buf.clone()
        for s, e, wd in ((lo_, o1, 0.0), (o1, hi_, E["wd"])):
            p[s:e], buf[s:e] = uo.sgd_ref(p[s:e], g[s:e], buf[s:e], nesterov=0, exact=True,
                                          **dict(E, wd=wd))
        g[lo_:hi_] = 0.0
        ux.same_bits(a.data.cpu(), ux.f32_of(p), f"step {step}: p", guard=0)
        ux.same_bits(opt.momentum_buffer.cpu(), ux.f32_of(buf), f"step {step}: buf", guard=0)
        ux.same_bits(a.grad.cpu(), ux.f32_of(g), f"step {step}: g", guard=0)
