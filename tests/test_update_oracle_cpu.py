"""tests/update_oracle.py proved without a GPU.

* The oracle's formula equals torch.optim.SGD on the CPU in fp64, bit for bit (plain, nesterov,
  momentum 0, wd 0), and ``bf16_rne_bits`` equals torch's fp32 -> bf16 conversion on the pattern
  set the GPU wire test uses.
* The exact recipe of tests/test_gpu_update_exact.py (lr 2**-2, momentum 2**-1, wd 2**-3,
  grad_scale 2**-1, integers in [-64, 64]) passes the oracle's "every intermediate is an fp32
  number" precondition for the two steps the GPU tests take (p is then a multiple of 2**-13
  below 2**8: 21 bits; a third step can need 27), and its results hold bf16 ties of both
  parities. The project's own hyperparameters fail the precondition, as they must.
* What the earlier checks miss: five local defects are injected into the REFERENCE's result (a
  stand-in for a kernel with that defect). ``allclose(rtol=1e-5, atol=1e-6)`` accepts a wrong last
  bit of p; ``cos > 0.99 and |norm ratio - 1| < 0.02`` (the only single-GPU check of the sharded
  update) accepts a tensor whose last three elements were never updated, a shard that lost one
  float4, a non-zero pad channel of Wc and a bf16 tie rounded away from zero. The bitwise
  comparison rejects all five.
"""
import numpy as np
import pytest
import torch

import update_oracle as uo
from exactness import int_tensor, mismatches

EXACT = dict(lr=2.0 ** -2, momentum=2.0 ** -1, wd=2.0 ** -3, grad_scale=2.0 ** -1)
PROJECT = dict(lr=0.1, momentum=0.9, wd=1e-4, grad_scale=0.5)


def test_bf16_rne_bits_matches_torch():
    u, s = uo.wire_patterns()
    for pat in (u, s, np.arange(0, 1 << 32, 65521, dtype=np.uint64).astype(np.uint32)):
        x = pat.view(np.float32)
        got = uo.bf16_rne_bits(x)
        want = uo.bf16_to_bits(torch.from_numpy(x.copy()).to(torch.bfloat16))
        nan = np.isnan(x)
        assert np.array_equal(got[~nan], want[~nan])
        assert bool(((got[nan] & 0x7f80) == 0x7f80).all() and ((got[nan] & 0x7f) != 0).all())
    assert uo.bf16_rne_bits(np.array([1.00390625], np.float32))[0] == 0x3f80   # tie, even: down
    assert uo.bf16_rne_bits(np.array([1.01171875], np.float32))[0] == 0x3f82   # tie, odd: up


@pytest.mark.parametrize("momentum,wd,nesterov", [(0.875, 3 / 128, False), (0.875, 3 / 128, True),
                                                  (0.0, 3 / 128, False), (0.875, 0.0, False),
                                                  (0.0, 0.0, False)])
def test_oracle_equals_torch_sgd_fp64(momentum, wd, nesterov):
    """Three steps against torch.optim.SGD in fp64. torch's CPU kernels contract a + alpha * b
    into one fused operation and the oracle does not, so bitwise equality is asked where fp64
    itself does not round: integer data and hyperparameters of three significant bits (lr 3/32,
    momentum 7/8, wd 3/128; about 12 more bits per step, 43 of fp64's 53 after three)."""
    g0 = torch.Generator().manual_seed(3)
    n = 1000
    lr = 3 / 32
    p = torch.randint(-64, 65, (n,), generator=g0).double()
    ref = torch.nn.Parameter(p.clone())
    opt = torch.optim.SGD([ref], lr=lr, momentum=momentum, weight_decay=wd, nesterov=nesterov,
                          foreach=False)
    buf = torch.zeros(n, dtype=torch.float64)
    for step in range(3):
        g = torch.randint(-64, 65, (n,), generator=g0).double()
        ref.grad = (g * 0.5).clone()   # torch has no grad_scale: 0.5 is exact
        opt.step()
        b_before = buf.clone()
        p, buf = uo.sgd_ref(p, g, buf, lr, momentum, wd, 0.5, nesterov)
        assert torch.equal(p, ref.detach()), step
        if momentum == 0.0:
            assert torch.equal(buf, b_before)  # untouched
        else:
            assert torch.equal(buf, opt.state[ref]["momentum_buffer"])


def _recipe(n, seed):
    return (int_tensor((n,), -64, 64, seed).double(), int_tensor((n,), -64, 64, seed + 1).double(),
            int_tensor((n,), -64, 64, seed + 2).double())


@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("momentum", [2.0 ** -1, 0.0])
def test_exact_recipe_two_steps(nesterov, momentum):
    h = dict(EXACT, momentum=momentum)
    p, g, buf = _recipe(20000, 40)
    for step in range(2):
        g = int_tensor((20000,), -64, 64, 50 + step).double()
        p, buf = uo.sgd_ref(p, g, buf, nesterov=nesterov, exact=True, **h)
    assert float(p.abs().max()) < 2.0 ** 8
    assert bool((p * 2.0 ** 13 == (p * 2.0 ** 13).round()).all())
    tie, odd = uo.is_tie(p)
    assert (tie & ~odd).any() and odd.any(), "the recipe must produce bf16 ties of both parities"


def test_exact_mode_refuses_values_that_round():
    p, g, buf = _recipe(1000, 40)
    with pytest.raises(AssertionError, match="not an fp32 number"):
        uo.sgd_ref(p, g, buf, nesterov=0, exact=True, **PROJECT)


def test_run_items_rules():
    """Skip, counter, signal and schedule rules of the fused launch, and the ownership of the Wt
    rows c >= Cr, on a small mixed table."""
    K, Cr, C, R = 8, 3, 8, 3
    n = 1024
    p, g, buf = _recipe(n, 60)
    d = [64, K, Cr, C, R, R, 1001, 1002, 0, 0, 0, 0]
    mem = {1001: np.full(K * R * R * C, 0x7fc5, np.uint16),
           1002: np.full(C * R * R * K, 0x7fc5, np.uint16)}
    items = uo.tile_items(0, d) + [[0, 512, 5, 0], [4, 600, 8, 0], [3, 700, 8, 4]]
    h = dict(EXACT, nesterov=0, zero_grad=1, delta=3, sched_advance=1)
    sched = dict(step=1, n=2, next=1, rates=[0.5, 0.25])
    kw = dict(mem=mem, shadow=np.full(n, 0x7fc5, np.uint16), slot=torch.full((64,), -1.0).double(),
              counter=10, done=0, signal=7, sched=sched, exact=True)
    o = uo.run_items(items, [d], p, g, buf, h, **kw)
    assert o["counter"] == 13 and o["done"] == 0 and o["signal"] == 8 and o["sched"]["next"] == 2
    wc = o["mem"][1001].reshape(K, R, R, C)
    wt = o["mem"][1002].reshape(C, R, R, K)
    assert (wc[..., Cr:] == 0).all() and (wt[Cr:] == 0x7fc5).all() and (wt[:Cr] != 0x7fc5).all()
    newp = o["p"][64:64 + K * Cr * R * R].view(K, Cr, R, R)
    assert np.array_equal(wc[..., :Cr], uo.bf16_bits_of(newp.permute(0, 2, 3, 1).contiguous()))
    assert np.array_equal(wt[:Cr], uo.bf16_bits_of(newp.permute(1, 2, 3, 0).contiguous()))
    assert bool((o["g"][600:608] == 0).all()) and bool((o["g"][512:517] == 0).all())
    assert torch.equal(o["g"][517:600], g[517:600]) and torch.equal(o["p"][517:700], p[517:700])
    assert torch.equal(o["slot"][4:12], o["p"][700:708]) and float(o["slot"][3]) == -1.0
    assert np.array_equal(o["shadow"][700:708], uo.bf16_bits_of(o["p"][700:708]))
    assert (np.delete(o["shadow"], np.arange(700, 708)) == 0x7fc5).all()
    s = uo.run_items(items, [d], p, g, buf, h, skip=1, **kw)
    assert s["counter"] == 13 and s["done"] == 0 and s["signal"] == 8 and s["sched"]["next"] == 2
    assert torch.equal(s["p"], p) and torch.equal(s["g"], g) and torch.equal(s["buf"], buf)
    assert all(np.array_equal(s["mem"][k], mem[k]) for k in mem)
    assert (s["shadow"] == 0x7fc5).all() and bool((s["slot"] == -1.0).all())
    # the abs pass bounds the signed pass
    t = uo.run_items(items, [d], p, g, buf, h, abs_pass=True, **kw)
    assert bool((t["p"] >= o["p"].abs()).all()) and bool((t["buf"] >= o["buf"].abs()).all())


@pytest.mark.parametrize("krsc", [0, 1])
def test_run_items_guard_skipped(krsc):
    """A guard-skipped launch: items 0-3 change nothing but g, which becomes +0 exactly where the
    normal launch with zero_grad clears it (and nowhere without zero_grad); items 4 and 5 run;
    counter, signal and staged step as in any step; the skip word keeps precedence."""
    K, Cr, C, R = 40, 3, 8, 3   # two tiles along K, channel padded
    n = 2048
    p, g, buf = _recipe(n, 70)
    g[g == 0] = 1.0   # every cleared element is then visible
    d = [64, K, Cr, C, R, R, 1001, 1002, krsc, 0, 0, 0]
    d2 = [1280, 4, 4, 4, 1, 1, 1003, 0, 0, 0, 0, 0]
    mem = {1001: np.full(K * R * R * C, 0x7fc5, np.uint16),
           1002: np.full(C * R * R * K, 0x7fc5, np.uint16), 1003: np.full(16, 0x7fc5, np.uint16)}
    items = uo.tile_items(0, d)[:1] + [[0, 1200, 5, 0], [4, 1216, 8, 0], [3, 1232, 8, 4],
                                       [2, 4, 8, 1], [5, 12, 4, 1]]
    sched = dict(step=1, n=2, next=1, rates=[0.5, 0.25])
    kw = dict(mem=mem, shadow=np.full(n, 0x7fc5, np.uint16), slot=torch.full((64,), -1.0).double(),
              counter=10, done=0, signal=7, sched=sched)
    for zg in (0, 1):
        h = dict(EXACT, nesterov=0, zero_grad=zg, delta=3, sched_advance=1)
        o = uo.run_items(items, [d, d2], p, g, buf, h, exact=True, **kw)
        s = uo.run_items(items, [d, d2], p, g, buf, h, guard_skipped=True, **kw)
        assert s["counter"] == 13 and s["done"] == 0 and s["signal"] == 8
        assert s["sched"]["next"] == 2
        assert torch.equal(s["p"], p) and torch.equal(s["buf"], buf)
        assert (s["shadow"] == 0x7fc5).all() and bool((s["slot"] == -1.0).all())
        assert all(np.array_equal(s["mem"][k], mem[k]) for k in (1001, 1002))
        # item 5 ran (the old masters' bf16), item 2 did not write its copy
        assert np.array_equal(s["mem"][1003][12:16], uo.bf16_bits_of(p[1292:1296]))
        assert (s["mem"][1003][:12] == 0x7fc5).all()
        # g: exactly what the normal launch leaves (item 4's range always, the rest with zero_grad)
        assert torch.equal(s["g"], o["g"])
        cleared = int((s["g"] == 0).sum())
        assert cleared == (8 + zg * (32 * Cr * R * R + 5 + 8 + 8))
        # the skip word keeps precedence
        w = uo.run_items(items, [d, d2], p, g, buf, h, guard_skipped=True, skip=1, **kw)
        assert torch.equal(w["g"], g) and np.array_equal(w["mem"][1003], mem[1003])


# ---------------------------------------------------------------------- what the old checks miss
def old_allclose(got, ref):
    return torch.allclose(got, ref, rtol=1e-5, atol=1e-6)


def old_cos_norm(got, ref):
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    cos = float(got @ ref / (got.norm() * ref.norm()))
    return cos > 0.99 and abs(float(got.norm() / ref.norm()) - 1.0) < 0.02


def _bound_case(n=4096):
    g0 = torch.Generator().manual_seed(9)
    p = torch.randn(n, generator=g0)
    g = torch.randn(n, generator=g0)
    buf = torch.randn(n, generator=g0)
    np_, nb = uo.sgd_ref(p.double(), g.double(), buf.double(), nesterov=0, **PROJECT)
    return p, np_.float(), nb.float()


def test_old_checks_miss_local_defects():
    p0, ref, _ = _bound_case()
    n = ref.numel()

    # 1. one wrong last bit of p: allclose(rtol=1e-5) spans about 170 half-ulps
    bad = ref.clone()
    i = int(ref.abs().argmax())
    bad[i] = torch.nextafter(ref[i], torch.tensor(float("inf")))
    assert old_allclose(bad, ref) and int(mismatches(bad, ref).sum()) == 1

    # 2. the last three elements of a tensor never updated (a lost scalar tail)
    bad = ref.clone()
    bad[-3:] = p0[-3:]
    assert old_cos_norm(bad, ref) and int(mismatches(bad, ref).sum()) == 3

    # 3. a shard that skips one float4
    bad = ref.clone()
    bad[1024:1028] = p0[1024:1028]
    assert old_cos_norm(bad, ref) and int(mismatches(bad, ref).sum()) == 4

    # 4. one pad channel of Wc left non-zero (K = 64, 3x3, Cr = 3 of C = 8)
    K, Cr, C, R = 64, 3, 8, 3
    w = ref[:K * Cr * R * R].numpy().copy()
    d = [0, K, Cr, C, R, R, 1, 0, 0, 0, 0, 0]
    wc, _ = uo.pack_ref(w, d, wc=np.full(K * R * R * C, 0x7fc5, np.uint16))
    badb = wc.copy().reshape(K, R, R, C)
    badb[5, 1, 2, Cr] = uo.bf16_rne_bits(np.array([0.5], np.float32))[0]
    a, b = uo.bits_to_bf16(badb.reshape(-1)), uo.bits_to_bf16(wc)
    assert old_cos_norm(a.float(), b.float()) and int(mismatches(a, b).sum()) == 1

    # 5. one bf16 tie rounded away from zero instead of to even
    x = ref.numpy().copy()
    x[7] = np.float32(1.00390625)   # 0x3f808000: half way, even neighbour below
    good = uo.bf16_rne_bits(x)
    away = good.copy()
    away[7] += 1
    assert good[7] == 0x3f80
    a, b = uo.bits_to_bf16(away), uo.bits_to_bf16(good)
    assert old_cos_norm(a.float(), b.float()) and int(mismatches(a, b).sum()) == 1
