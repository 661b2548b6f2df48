"""CPU oracle of the AdamW rule of the fused update launch (csrc/kernels/api.h AdamArgs,
optim/adamw.py), written down again in plain fp64 torch from the formula, next to
tests/update_oracle.py (whose item tables and bf16 rounding the AdamW tests reuse).

Per element, all in fp64 here, from fp32-valued hyper-parameters and table entries:

    G   = g * gs
    m'  = m + omb1 * (G - m)
    v'  = (omb2 * G) * G + beta2 * v
    den = sqrt(v') * a2 + eps
    u   = m' / den
    p'  = (p - lw * p) - la * u            la = float32(lr * a1), lw = float32(lr * wd)

``hp``: dict of lr, wd, grad_scale, omb1, beta2, omb2, eps, a1, a2. ``la`` and ``lw`` are the one
fp32 product each that the kernel takes once per block; ``table_exact=True`` takes them in fp64
instead (the comparison with real arithmetic counts their rounding in its bound).

Exact mode (``exact=True``): every intermediate -- G, G - m, m', omb2 * G, beta2 * v, v', its
square root, den, u, lr * a1, lr * wd, p - lw * p, p' -- is asserted to be an fp32 number. Then
no fp32 operation rounds, fused or not, provided sqrt and / are correctly rounded, and a correct
kernel returns these values bit for bit.

``adamw_abs`` runs the same formula on the magnitudes and returns the T terms of the bounds:
T_m = |m| + omb1 (|G| + |m|), v' (all its terms are non-negative: v' itself), den, and
T_u = T_m / den.
"""
import numpy as np
import torch

from update_oracle import f32, is_f32

KEYS = ("lr", "wd", "grad_scale", "omb1", "beta2", "omb2", "eps", "a1", "a2")


def hyper(lr, wd, grad_scale, beta1, beta2, eps, a1, a2):
    """``hp`` from the optimizer's hyper-parameters, each at the fp32 value the kernel gets
    (1 - beta in fp64, rounded once)."""
    return dict(lr=f32(lr), wd=f32(wd), grad_scale=f32(grad_scale), omb1=f32(1.0 - beta1),
                beta2=f32(beta2), omb2=f32(1.0 - beta2), eps=f32(eps), a1=f32(a1), a2=f32(a2))


def bias64(beta1, beta2, t):
    """{a1, a2} of step t in fp64."""
    return 1.0 / (1.0 - beta1 ** t), 1.0 / np.sqrt(1.0 - beta2 ** t)


def adamw_ref(p, g, m, v, hp, exact=False, table_exact=False):
    """New (p, m, v) in fp64."""
    assert all(f32(hp[k]) == hp[k] for k in KEYS), "hyper-parameters must be fp32 values"
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    la, lw = hp["lr"] * hp["a1"], hp["lr"] * hp["wd"]
    if exact:
        assert f32(la) == la and f32(lw) == lw, "adamw_ref exact mode: lr * a1 or lr * wd rounds"
    if not table_exact:
        la, lw = f32(la), f32(lw)
    steps = []
    G = g * hp["grad_scale"]
    steps.append(("g*gs", G))
    d = G - m
    steps.append(("G-m", d))
    nm = m + hp["omb1"] * d
    steps.append(("m+omb1*(G-m)", nm))
    w = hp["omb2"] * G
    steps.append(("omb2*G", w))
    bv = hp["beta2"] * v
    steps.append(("beta2*v", bv))
    nv = w * G + bv
    steps.append(("omb2*G*G+beta2*v", nv))
    s = nv.sqrt()
    steps.append(("sqrt(v')", s))
    den = s * hp["a2"] + hp["eps"]
    steps.append(("sqrt(v')*a2+eps", den))
    u = nm / den
    steps.append(("m'/den", u))
    q = p - lw * p
    steps.append(("p-lw*p", q))
    np_ = q - la * u
    steps.append(("q-la*u", np_))
    if exact:
        assert bool((s * s == nv).all()), "adamw_ref exact mode: v' is not a perfect square"
        for name, x in steps:
            assert bool(is_f32(x).all()), f"adamw_ref exact mode: {name} is not an fp32 number"
    return np_, nm, nv


def adamw_abs(p, g, m, v, hp):
    """The T terms: dict of T_m, v (= v'), den, T_u = T_m / den, p = |p|, la, lw."""
    p, g, m, v = p.double().abs(), g.double().abs(), m.double().abs(), v.double().abs()
    G = g * abs(hp["grad_scale"])
    Tm = m + hp["omb1"] * (G + m)
    nv = hp["omb2"] * G * G + hp["beta2"] * v
    den = nv.sqrt() * hp["a2"] + hp["eps"]
    return dict(T_m=Tm, v=nv, den=den, T_u=Tm / den, p=p, la=abs(hp["lr"] * hp["a1"]),
                lw=abs(hp["lr"] * hp["wd"]))


def bounds(T, eps, table_roundings=0):
    """First-order bounds of one step from exact inputs, eps = 2**-24 (derivation: the docstring
    of tests/test_adamw_cpu.py test_cpu_path_against_real_arithmetic):
        m'  3 eps T_m;   v'  4 eps v';   p'  eps (3 (1 + lw) |p| + (10 + table_roundings) la T_u)
    plus, per rounding, half the smallest fp32 subnormal, 2**-150: below the normal range a
    rounding errs by that much and not by eps of its result (G * G of a gradient below 1e-19)."""
    tiny = 2.0 ** -150
    return dict(m=3 * eps * T["T_m"] + 3 * tiny, v=4 * eps * T["v"] + 4 * tiny,
                p=eps * (3 * (1 + T["lw"]) * T["p"] + (10 + table_roundings) * T["la"] * T["T_u"])
                + (13 + table_roundings) * tiny)
