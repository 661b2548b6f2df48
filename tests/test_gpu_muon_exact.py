"""The Muon kernels (csrc/kernels/muon.hip, the MUON items of optim.hip sgd_pack_kernel) bit for
bit against fp64 / numpy oracles, on the guard-band convention of tests/test_gpu_update_exact.py:
a NaN pattern around every buffer, WHOLE buffers compared.

Exact mode. GEMM operands are integers in {-2..2}, non-zero at no more than 32 reduction indices
(spread over every k-step), alpha and beta powers of two: every sum stays below 2^24 and every
result is a multiple of 1/2 below 128, a bf16 number (asserted on the reference). Stage: g and m
multiples of 4, mu = gs = 1/2, so d is an integer with |d| <= 28 and a chunk's sum below 2^24.
"""
import numpy as np
import pytest
import torch

import test_gpu_ema_exact as ex
import test_gpu_update_exact as ux
import update_oracle as uo
from ddp_amd.optim import muon as mu
from exactness import int_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
Buf, same_bits, BF = ux.Buf, ux.same_bits, torch.bfloat16


def _ints(shape, seed, keep_k=None, axis=1):
    t = int_tensor(shape, -2, 2, seed)
    if keep_k is not None:  # zero all but 32 reduction indices
        k = shape[axis]
        idx = torch.randperm(k, generator=torch.Generator().manual_seed(seed))[:32]
        mask = torch.zeros(k)
        mask[idx] = 1
        t = t * (mask[None, :] if axis == 1 else mask[:, None])
    return t


def _padded(t, rows, cols):
    out = torch.zeros(rows, cols)
    out[:t.shape[0], :t.shape[1]] = t
    return out


# (form, [(m, n, k, folded), ...]): one grouped launch over the listed tensors. nt is X X^T and sym
# the NN product A A + E of a symmetric A (n = m, tiles on and above the diagonal, mirrored).
# k-steps 1, 2, 4 (one per wave), 7 (two rounds, the second with one wave idle); 27 -> 32 and
# 40 x 72 -> 64 x 96 only through padding. The folded tensor takes s0 = 1 / 4 with the powers
# production uses: (2, -) for nt, (1, 1) for the others.
def _shapes(f):
    sq = f in ("nt", "sym")
    return ([(32, 32, 32, False)], [(64, 64, 64, False)],
            [(27, 27, 64, False)] if f == "nt" else [(27, 27 if sq else 64, 27, False)],
            [(40, 40 if sq else 72, 40 if f == "sym" else 200, False), (64, 64, 64 if f == "sym" else 128, True)])


@pytest.mark.parametrize("form,tensors", [(f, t) for f in ("nt", "nn", "nne", "sym") for t in _shapes(f)])
def test_gemm_exact(native_ext, form, tensors):
    part = Buf(4, fill=torch.tensor([4.0, 12.0, 0.0, 0.0]))  # S = 16: s0 = 1 / 4
    rows, items, out = [], [], []
    for q, (m, n, k, fold) in enumerate(tensors):
        mp, np_, kp = mu._pad(m), mu._pad(n), mu._pad(k)
        A = _ints((m, k), 10 * q + 1, keep_k=True)
        if form == "sym":
            A = torch.triu(A) + torch.triu(A, 1).t()
            keep = (A.abs().sum(0) > 0).float().cumsum(0) <= 32  # at most 32 reduction indices
            A = A * keep[None, :] * keep[:, None]
        A = _padded(A, mp, kp)
        B = A if form in ("nt", "sym") else _padded(_ints((k, n), 10 * q + 2, keep_k=True, axis=0), kp, np_)
        op = A.double() @ (B.double().t() if form == "nt" else B.double())
        E = A if form == "sym" else _padded(_ints((m, n), 10 * q + 3), mp, np_) if form == "nne" else None
        pa, pb = (2, 0) if form == "nt" else (1, 1)
        alpha, beta = (0.5 * 4 ** pa, 2.0 * 4 ** pb) if fold else (0.5, 2.0)
        ref = 0.5 * op + (2.0 * E.double() if E is not None else 0.0)
        assert float(ref.abs().max()) < 128 and bool((ref * 2 == (ref * 2).round()).all())
        dA, dB, dD = Buf(mp * kp, BF, A), Buf(B.numel(), BF, B), Buf(mp * np_, BF)
        dE = dA if form == "sym" else Buf(mp * np_, BF, E) if E is not None else None
        out.append((dD, dD.host(), ref, dA, dB, dE))
        rows.append(dict(a=dA.ptr, b=dA.ptr if form in ("nt", "sym") else dB.ptr, e=dE.ptr if dE else 0,
                         d=dD.ptr, lda=kp, ldb=kp if form != "nn" and form != "nne" else np_, ldd=np_,
                         ksteps=kp // 32, alpha=alpha, beta=beta, rows=m, cols=n,
                         **(dict(norm0=0, norm_n=2, alpha_pow=pa, beta_pow=pb) if fold else {})))
        items += mu.tile_items(q, mp, np_, form in ("nt", "sym"))
    table = mu.device_table(rows, mu.GEMM_DTYPE, DEV)
    it = torch.tensor(items, dtype=torch.int32, device=DEV)
    native_ext.muon_gemm(it.data_ptr(), len(items), table.data_ptr(), part.ptr, int(form != "nt"), ux.stream())
    torch.cuda.synchronize()
    for q, (dD, before, ref, *_) in enumerate(out):
        same_bits(dD.host(), dD.expect(before, (ref + 0.0).float()), f"{form} tensor {q}: D")


# test_gpu_lamb_exact.NormsCase's arena: 4 x 2798 (a full and a partial chunk, rows that end inside a
# float4), 110 x 3 (tall: staged transposed; the scalar tail), 8 x 1024 (its chunk is NOT in the launch)
STAGE_SHAPES = ((4, 2798), (110, 3), (8, 1024))


@pytest.mark.parametrize("nesterov,guard", [(1, False), (0, False), (1, True)])
def test_stage_exact(native_ext, nesterov, guard):
    """guard: clip partials {4, 0, 12}, max_norm 2: c = 1 / 2, so gs c = 1 / 4 and d a multiple of 1 / 4."""
    offs, off = [], 64
    for K, r in STAGE_SHAPES:
        offs.append(off)
        off += (K * r + 63) // 64 * 64 + 64
    gb, mb = (Buf(off, fill=4 * int_tensor((off,), -4, 4, 71 + i)) for i in range(2))
    part, rows, items, xs, c = Buf(7), [], [], [], 1
    for q, ((K, r), o) in enumerate(zip(STAGE_SHAPES, offs)):
        t = K > r
        mp, np_ = (mu._pad(r), mu._pad(K)) if t else (mu._pad(K), mu._pad(r))
        x = Buf(mp * np_, BF, torch.zeros(mp * np_))
        xs.append((x, x.host(), mp, np_, t, o, K, r))
        rows.append(dict(p_offset=o, x=x.ptr, pitch=np_, rest=r, transposed=int(t), scale=1.0))
        items += [[o + s0, min(8192, K * r - s0), c + j, q] for j, s0 in enumerate(range(0, K * r, 8192))]
        c += -(-K * r // 8192) + (q == 1)
    items = items[:3]  # global chunks 1, 2, 3 of 7 slots; the third tensor stays out
    g, m = gb.inner.cpu().double(), mb.inner.cpu().double()
    before = dict(g=gb.host(), m=mb.host(), part=part.host())
    table = mu.device_table(rows, mu.TENSOR_DTYPE, DEV)
    it = torch.tensor(items, dtype=torch.int32, device=DEV)
    kw, keep = ex.guard_kw([4.0, 0.0, 12.0], 2.0, 1 | 2 | 4) if guard else ({}, None)
    kw.pop("clip_stats", None)
    native_ext.muon_stage(it.data_ptr(), len(items), table.data_ptr(), gb.ptr, mb.ptr, 0.5, 0.5, nesterov,
                          part.ptr, ux.stream(), **kw)
    torch.cuda.synchronize()
    G = g * (0.25 if guard else 0.5)
    m1 = 0.5 * m + G
    d = 0.5 * m1 + G if nesterov else m1
    assert bool((d * 4 == (d * 4).round()).all()) and float(d.abs().max()) <= 28
    want = before["part"][ux.GUARD:ux.GUARD + 7].clone()
    for o, n, ch, _ in items:
        want[ch] = float((d[o:o + n] ** 2).sum())
        assert float(want[ch]) == float((d[o:o + n] ** 2).sum())
    same_bits(part.host(), part.expect(before["part"], want), "partials")
    same_bits(gb.host(), before["g"], "g untouched")
    same_bits(mb.host(), before["m"], "m untouched")
    for q, (x, x0, mp, np_, t, o, K, r) in enumerate(xs):
        M = d[o:o + K * r].reshape(K, r)
        w = _padded(M.t() if t else M, mp, np_) if q < 2 else torch.zeros(mp, np_)
        same_bits(x.host(), x.expect(x0, (w + 0.0).float()), f"staged matrix {q}")


def test_update_items_exact(native_ext):
    """One launch, zero_grad on: a 16 x 3 x 3 x 8 conv (item 2, wide), the channel-padded 64 x 3 x 3 x 3
    conv (items 1, tall: O read transposed) and a bare 96 x 2 x 2 x 8 tensor (item 0, tall) take the
    Muon rule with O handed in as even integers, lr = 2^-2, wd = 2^-3, mu = 2^-1, s = 2; a plain
    item 0 in the same launch is sgd_pack_kernel's own, as update_oracle.run_items has it."""
    h = dict(ux.EXACT, nesterov=True, zero_grad=1)
    shapes = [(16, 8, 8, 3), (64, 3, 8, 3), (96, 32, 32, 1)]  # K, Cr, C, R (S = R)
    n_el = [K * Cr * R * R for K, Cr, C, R in shapes]
    offs = [0, 1152, 1152 + 1728]
    plain0 = offs[2] + n_el[2]
    A = ux.Arena(plain0 + 300, 5)
    A.p.set(32 * int_tensor((A.n,), -4, 4, 6))
    mem = {q + 1: Buf(K * C * R * R, BF) for q, (K, Cr, C, R) in enumerate(shapes[:2])}
    rows = [[offs[q], K, Cr, C, R, R, q + 1, 0, 1, 0, 0, 0] for q, (K, Cr, C, R) in enumerate(shapes[:2])]
    dev_rows = [r[:6] + [mem[r[6]].ptr] + r[7:] for r in rows]
    items = [[2, 0, 1152, 0]] + uo.tile_items(1, rows[1]) + [[0, offs[2], n_el[2], 0], [0, plain0, 300, 0]]
    side = [0] + [1] * (len(items) - 3) + [2, -1]
    marked = [[k | (mu.ITEM_MUON if s >= 0 else 0), a, b, c] for (k, a, b, c), s in zip(items, side)]
    outs, O = [], []
    for q, (K, Cr, C, R) in enumerate(shapes):
        rest = n_el[q] // K
        t = K > rest
        mp, np_ = (mu._pad(rest), mu._pad(K)) if t else (mu._pad(K), mu._pad(rest))
        o = 2 * int_tensor((K, rest), -3, 3, 20 + q)
        O.append(o)
        x = Buf(mp * np_, BF, _padded(o.t() if t else o, mp, np_))
        outs.append((x, dict(p_offset=offs[q], x=x.ptr, pitch=np_, rest=rest, transposed=int(t), scale=2.0)))
    table = mu.device_table([r for _, r in outs], mu.TENSOR_DTYPE, DEV)
    sd = torch.tensor(side, dtype=torch.int32, device=DEV)
    before = {k: b.host() for k, b in dict(p=A.p, g=A.g, buf=A.buf, m1=mem[1], m2=mem[2]).items()}
    p, g, buf = A.host64()
    o = uo.run_items(items, rows, p, g, buf, h, exact=True, mem={q: b.np_bits() for q, b in mem.items()})
    for q in range(3):  # the Muon rule over the three tensors, in fp64
        sl = slice(offs[q], offs[q] + n_el[q])
        G = g[sl] * h["grad_scale"]
        o["buf"][sl] = h["momentum"] * buf[sl] + G
        o["p"][sl] = p[sl] - h["lr"] * h["wd"] * p[sl] - h["lr"] * 2.0 * O[q].double().reshape(-1)
        if q < 2:
            uo.pack_ref(o["p"].float().numpy(), rows[q], wc=o["mem"][q + 1])
    ux.launch(native_ext, marked, dev_rows, A, h, muon_side=sd.data_ptr(), muon_tensors=table.data_ptr())
    for name, b, want in (("p", A.p, o["p"]), ("buf", A.buf, o["buf"]), ("g", A.g, o["g"])):
        same_bits(b.host(), b.expect(before[name], ux.f32_of(want)), name)
    for q in (1, 2):
        same_bits(mem[q].host(), mem[q].expect(before[f"m{q}"], ux.bf16_of(o["mem"][q])), f"bf16 copy {q}")
