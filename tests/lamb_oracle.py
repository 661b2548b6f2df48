"""CPU oracle of the LAMB rule (csrc/kernels/api.h LambArgs, optim/lamb.py), written down again in
plain fp64 torch on top of tests/adamw_oracle.py (``hp``, the bias table, the first five lines).

Per element, all in fp64 here, from fp32-valued hyper-parameters and table entries:

    m', v', u          as adamw_oracle.adamw_ref (G, m', v', den, u)
    r   = wd * p + a1 * u
    per chunk / tensor: sum p^2, sum r^2;  wn = sqrt(sum p^2), rn = sqrt(sum r^2)
    trust = wn / rn    if adapted and wn > 0 and rn > 0, else 1
    p'  = p - lt * r                      lt = float32(lr * trust), the kernel's one product

Exact mode (``exact=True``): every intermediate is asserted to be an fp32 number: AdamW's, a1 * u,
wd * p, r, every p^2 and r^2, and every partial sum IN ANY ORDER: all terms are integer multiples
of one unit (the smallest non-zero term's) and the total, in that unit, stays below 2^24, so no
order of fp32 additions rounds. Then a correct kernel returns these values bit for bit.

``lamb_abs`` runs the formula on the magnitudes and returns the T terms of the bounds; ``bounds``
and ``trust_rtol`` count the roundings (derivations in their docstrings).
"""
import math

import numpy as np

import torch

import adamw_oracle as ao
from update_oracle import f32, is_f32

TINY = 2.0 ** -150


def direction(p, g, m, v, hp, exact=False):
    """(r, m', v') in fp64: AdamW's first five lines and the update direction."""
    assert all(f32(hp[k]) == hp[k] for k in ao.KEYS), "hyper-parameters must be fp32 values"
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    steps = []
    G = g * hp["grad_scale"]
    d = G - m
    nm = m + hp["omb1"] * d
    w = hp["omb2"] * G
    bv = hp["beta2"] * v
    nv = w * G + bv
    s = nv.sqrt()
    den = s * hp["a2"] + hp["eps"]
    u = nm / den
    au = hp["a1"] * u
    wp = hp["wd"] * p
    r = wp + au
    steps += [("g*gs", G), ("G-m", d), ("m'", nm), ("omb2*G", w), ("beta2*v", bv), ("v'", nv),
              ("sqrt(v')", s), ("den", den), ("u", u), ("a1*u", au), ("wd*p", wp), ("r", r)]
    if exact:
        assert bool((s * s == nv).all()), "lamb oracle exact mode: v' is not a perfect square"
        for name, x in steps:
            assert bool(is_f32(x).all()), f"lamb oracle exact mode: {name} is not an fp32 number"
    return r, nm, nv


def sum_sq(x, exact=False):
    """Sum of squares in fp64; ``exact``: no fp32 summation order rounds (module docstring)."""
    x = x.double().reshape(-1)
    sq = x * x
    total = float(sq.sum())
    if exact and total > 0:
        assert bool(is_f32(sq).all()), "lamb oracle exact mode: a square is not an fp32 number"
        # the unit: the lowest set bit over all terms (every term and every partial sum is an
        # integer number of units)
        mant, expo = np.frexp(sq[sq > 0].numpy())
        M = (mant * 2.0 ** 53).astype(np.int64)
        unit = float(((M & -M).astype(np.float64) * np.exp2(expo.astype(np.float64) - 53)).min())
        assert total / unit < 2.0 ** 24, f"lamb oracle exact mode: sum {total / unit} units >= 2^24"
    return total


def chunk_sums(p, r, chunk=8192, exact=False):
    """Per chunk of one tensor's elements {sum p^2, sum r^2}: float64 [chunks][2]."""
    p, r = p.reshape(-1), r.reshape(-1)
    return torch.tensor([[sum_sq(p[s:s + chunk], exact), sum_sq(r[s:s + chunk], exact)]
                         for s in range(0, p.numel(), chunk)], dtype=torch.float64)


def trust_of(sp, sr, adapted=True, exact=False):
    """wn / rn in fp64 from the two sums, or 1."""
    if not adapted or not (sp > 0 and sr > 0):
        return 1.0
    wn, rn = math.sqrt(sp), math.sqrt(sr)
    t = wn / rn
    if exact:
        assert wn * wn == sp and rn * rn == sr and f32(t) == t, "lamb oracle exact mode: trust rounds"
    return t


def apply(p, r, hp, trust, exact=False):
    """p' = p - float32(lr * trust) * r with the fp32 ``trust`` given (the oracle's own, or the
    one the device stored)."""
    assert f32(trust) == trust, "trust must be an fp32 value"
    lt = hp["lr"] * trust
    if exact:
        assert f32(lt) == lt, "lamb oracle exact mode: lr * trust rounds"
    out = p.double() - f32(lt) * r
    if exact:
        assert bool(is_f32(out).all()), "lamb oracle exact mode: p' is not an fp32 number"
    return out


def lamb_ref(p, g, m, v, hp, adapted=True, trust=None, exact=False):
    """One tensor: (p', m', v', trust, r). ``trust``: use this fp32 ratio instead of the oracle's."""
    r, nm, nv = direction(p, g, m, v, hp, exact)
    if trust is None:
        trust = f32(trust_of(sum_sq(p, exact), sum_sq(r, exact), adapted, exact))
    return apply(p, r, hp, trust, exact), nm, nv, trust, r


def lamb_abs(p, g, m, v, hp):
    """adamw_abs plus T_r = wd |p| + a1 T_u."""
    T = ao.adamw_abs(p, g, m, v, hp)
    T["T_r"] = abs(hp["wd"]) * T["p"] + abs(hp["a1"]) * T["T_u"]
    return T


def bounds(T, eps, lt):
    """First-order bounds of one step from exact inputs and an exact fp32 trust, eps = 2**-24,
    lt = lr * trust. m' and v' are AdamW's (3 eps T_m, 4 eps v'). With T_u = T_m / den:
        u   = fl(m' / den)           8 eps T_u          (adamw_oracle.bounds, no table roundings)
        a1 u                         9 eps a1 T_u
        r   = fma(wd, p, a1 u)       9 eps a1 T_u + eps (wd |p| + a1 T_u) <= 10 eps T_r  =: E_r
        lt' = fl(lr trust)           1 eps relative
        p'  = fma(-lt', r, p)        lt (E_r + eps T_r) + eps (|p| + lt T_r) <= eps (|p| + 12 lt T_r)
    plus half the smallest subnormal per rounding (adamw_oracle.bounds)."""
    b = ao.bounds(T, eps)
    return dict(m=b["m"], v=b["v"], r=10 * eps * T["T_r"] + 11 * TINY,
                p=eps * (T["p"] + 12 * abs(lt) * T["T_r"]) + 13 * TINY)


# Longest serial chain of rounded additions behind one tensor's sum (tests/test_gpu_lars.py CHAIN):
# 33 fmas per thread, wave_sum 6, four wave results 3, in the update's prologue 1 + wave_sum 6.
CHAIN = 33 + 6 + 3 + 1 + 6


def trust_rtol(r, T_r, eps):
    """Relative bound of the device's wn / rn against fp64, from exact inputs.
      sum p^2: non-negative terms, CHAIN additions                    CHAIN eps relative
      sum r^2: each r is off by E_r <= 10 eps T_r (``bounds``; r may cancel, so the error is not
               relative to r): |sum fl(r)^2 - sum r^2| <= 2 sum |r| E_r, plus the chain
               -> (CHAIN + 20 sum(|r| T_r) / sum r^2) eps relative
      the square roots halve both; sqrt, sqrt and the division round once each: + 3 eps."""
    r, T_r = r.double().reshape(-1), T_r.double().reshape(-1)
    amp = float((r.abs() * T_r).sum() / (r * r).sum())
    return (0.5 * CHAIN + 0.5 * (CHAIN + 20 * amp) + 3) * eps
