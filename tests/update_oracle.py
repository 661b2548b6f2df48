"""CPU oracle of the update path: the SGD formula, the bf16 rounding and the work-item tables of
the fused SGD + re-pack launch, written down again from the comments of csrc/kernels/optim.hip in
plain fp64 torch / numpy. It imports nothing native and is no translation of the kernels: every
item is a handful of slice assignments on views of the arena.

Formula (header of optim.hip), per element, all in fp64 here:

    d = g * grad_scale + wd * p
    momentum != 0:  buf = momentum * buf + d ;  d = nesterov ? d + momentum * buf : buf
    momentum == 0:  buf is left alone
    p = p - lr * d

Exact mode (``exact=True``): the oracle asserts that every intermediate -- g * grad_scale,
wd * p + g * grad_scale, momentum * buf + d, the nesterov sum, p - lr * d -- is an fp32 number.
Then no operation of an fp32 implementation rounds, fused multiply-add or not, so any correct
kernel returns these values bit for bit. Bound mode: ``sgd_abs`` runs the same formula on the
magnitudes with +lr; its results T bound every partial sum behind an output, and a kernel with R
fp32 roundings on the path to it errs by at most R * 2**-24 * T.

Buffers: ``p``, ``g``, ``buf``, ``slot`` are flat fp64 torch tensors (the arena), the bf16
operand copies and ``shadow`` are flat numpy uint16 arrays of bit patterns. ``run_items`` copies
everything it is given and returns the new state; nothing is modified in place.
"""
import numpy as np
import torch


def f32(x):
    """The fp32 value a kernel argument carries, as a Python float."""
    return float(np.float32(x))


def is_f32(x):
    """Elementwise: is this fp64 value an fp32 number?"""
    return x.float().double() == x


def tile_dims(RS):
    """K x C extent of a tile item by filter size (must equal native sgd_tile_dims)."""
    if RS == 1:
        return 64, 64
    if RS <= 9:
        return 32, 32
    return 8, 16


# ------------------------------------------------------------------------------------- bf16
def bf16_rne_bits(x):
    """float32 array -> uint16 bf16 bit patterns, round to nearest even by the integer formula
    (u + 0x7fff + ((u >> 16) & 1)) >> 16; a NaN maps to a NaN (0x7fc0 with the input's sign)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7fffffff) > 0x7f800000
    return np.where(nan, ((u >> 16) & 0x8000 | 0x7fc0).astype(np.uint16), r)


def bf16_bits_of(t64):
    """fp64 torch values that are fp32 numbers -> bf16 bits (zeros taken as +0, as the kernels'
    sums give them)."""
    f = (t64 + 0.0).float()
    assert bool((f.double() == t64).all()), "bf16_bits_of: the values are not fp32 numbers"
    return bf16_rne_bits(f.contiguous().numpy())


def bits_to_bf16(bits):
    """uint16 numpy bit patterns -> torch.bfloat16 tensor (for exactness.mismatches)."""
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16)


def bf16_to_bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def is_tie(t64):
    """Values exactly half way between two bf16 numbers, and the parity of the lower neighbour's
    last kept bit: returns (tie mask, odd mask) as numpy arrays."""
    u = t64.float().contiguous().numpy().view(np.uint32)
    tie = (u & 0xffff) == 0x8000
    return tie, tie & (((u >> 16) & 1) == 1)


def wire_patterns():
    """fp32 bit patterns of the bf16 conversion tests: {upper 16 bits} x {lower 16 bits in 0x0000,
    0x0001, 0x7fff, 0x8000, 0x8001, 0xffff}. The upper list has both signs of zero, the smallest
    and largest normals, 0x3f7f (the carry runs into the exponent), 0x7f7f (rounds to inf), inf,
    NaNs, even and odd last kept bits, subnormals and 64 seeded random values. Returns (zeros,
    normals, inf and NaN; subnormals) as uint32 arrays."""
    rng = np.random.RandomState(5)
    hi = [0x0000, 0x8000, 0x0080, 0x8080, 0x7f7f, 0xff7f, 0x3f7f, 0xbf7f, 0x7f80, 0xff80,
          0x7fc0, 0xffc0, 0x7f81, 0x7fff, 0xffa5, 0x3f80, 0x3f81, 0x4000, 0x4001, 0xc2fe, 0xc2ff,
          0x0001, 0x8001, 0x007f, 0x807f, 0x0040, 0x8040]
    hi += [int(v) for v in rng.randint(0x0080, 0x7f80, 64)]
    lo = [0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff]
    u = np.array([(h << 16) | l for h in hi for l in lo], dtype=np.uint32)
    sub = ((u & 0x7f800000) == 0) & ((u & 0x007fffff) != 0)
    return u[~sub], u[sub]


# ------------------------------------------------------------------------------------- SGD
def sgd_ref(p, g, buf, lr, momentum, wd, grad_scale, nesterov, exact=False):
    """New (p, buf) in fp64. ``lr`` ... ``grad_scale`` are taken at their fp32 values, as the
    kernels receive them. ``exact``: assert that no intermediate needs rounding in fp32."""
    lr, momentum, wd, grad_scale = f32(lr), f32(momentum), f32(wd), f32(grad_scale)
    p, g, buf = p.double(), g.double(), buf.double()
    steps = []
    gs = g * grad_scale
    steps.append(("g*gs", gs))
    d = wd * p + gs
    steps.append(("wd*p+g*gs", d))
    nb = buf
    if momentum != 0.0:
        nb = momentum * buf + d
        steps.append(("m*b+d", nb))
        if nesterov:
            d = d + momentum * nb
            steps.append(("d+m*b", d))
        else:
            d = nb
    np_ = p - lr * d
    steps.append(("p-lr*d", np_))
    if exact:
        for name, v in steps:
            assert bool(is_f32(v).all()), f"sgd_ref exact mode: {name} is not an fp32 number"
    return np_, nb.clone()


def sgd_abs(p, g, buf, lr, momentum, wd, grad_scale, nesterov):
    """The formula on the magnitudes with +lr: (T_p, T_buf), the sums of magnitudes behind the
    new p and the new buf."""
    return sgd_ref(p.abs(), g.abs(), buf.abs(), -abs(f32(lr)), abs(f32(momentum)), abs(f32(wd)),
                   abs(f32(grad_scale)), nesterov)


# ------------------------------------------------------------------------------------- tables
def _master_view(t, d):
    """The [K][R][S][Cr] view of a conv master inside the flat tensor ``t`` (writable)."""
    off, K, Cr, R, S, krsc = int(d[0]), int(d[1]), int(d[2]), int(d[4]), int(d[5]), int(d[8])
    flat = t[off:off + K * Cr * R * S]
    if krsc:
        return flat.view(K, R, S, Cr)
    return flat.view(K, Cr, R, S).permute(0, 2, 3, 1)


def pack_ref(p32, d, wc=None, wt=None):
    """pack_conv_weights of one descriptor from the fp32 arena ``p32`` (numpy float32, flat):
    Wc [K][R][S][C] with +0 in the channels c >= Cr; Wt [C][R][S][K] with +0 in ITS rows
    c >= Cr (the stand-alone pack writes them, unlike a tile item). Writes into the given uint16
    arrays (flat) and returns them."""
    K, Cr, C, R, S = (int(d[i]) for i in (1, 2, 3, 4, 5))
    m = _master_view(torch.from_numpy(p32), d).contiguous().numpy()
    bits = bf16_rne_bits(m)
    if wc is not None:
        v = wc[:K * R * S * C].reshape(K, R, S, C)
        v[...] = 0
        v[..., :Cr] = bits
    if wt is not None:
        v = wt[:C * R * S * K].reshape(C, R, S, K)
        v[...] = 0
        v[:Cr] = bits.transpose(3, 1, 2, 0)
    return wc, wt


def lr_of(hyper, sched):
    """This launch's learning rate: the schedule's entry of the current step (clamped to the
    table's last), else the immediate value."""
    if sched is None:
        return hyper["lr"]
    r = sched["rates"]
    return float(r[min(int(sched["step"]), len(r) - 1)])


def run_items(items, descs, p, g, buf, hyper, mem=None, shadow=None, slot=None, skip=0,
              counter=None, done=None, signal=None, sched=None, exact=False, pack_source=None,
              abs_pass=False, guard_skipped=False):
    """One fused launch. ``items``: rows of 4 ints; ``descs``: rows of 12 ints {p_offset, K, Cr,
    C, R, S, wc, wt, krsc, -, -, -} whose wc / wt entries are keys into ``mem`` (the device
    pointers on the GPU); ``hyper``: lr, momentum, wd, grad_scale, nesterov, zero_grad, delta,
    sched_advance. ``pack_source``: an fp32 numpy image of a kernel's own new arena -- the bf16
    copies are then taken from it (bound mode: they are a pure function of what the kernel
    stored). ``abs_pass``: run ``sgd_abs`` instead (T of every element; bf16 copies untouched).

    Item 0 {0, off, cnt, -}: plain chunk.  Item 2 {2, rel, cnt, desc}: chunk of a conv master +
    its Wc in the same order.  Item 1 {1, desc, k0, c0}: a TK x TC tile; Wc gets +0 in the tile's
    channels c >= Cr; Wt (optional) only its rows c < Cr -- a tile item never touches the Wt rows
    c >= Cr.  Item 3 {3, off, cnt, slot_off | -1}: update, shadow[off + i] = bf16(new p),
    slot[slot_off + i] = new p.  Item 4 {4, off, cnt, -}: clear gradients.  Item 5 {5, rel, cnt,
    desc}: bf16 copy only. zero_grad writes +0. counter += delta even when skipped; a non-zero
    skip word leaves p, g, buf, every bf16 copy, shadow and slot unchanged; with a signal, done is
    0 afterwards and the signal one higher, skipped or not; with a schedule and sched_advance,
    next == step + 1, skipped or not.

    ``guard_skipped``: the gradient guard found a non-finite norm (optim.hip ClipArgs flag 2).
    Items 0-3 then change nothing but g, which becomes +0 over exactly the range the update
    covers, and only with zero_grad; items 4 and 5 run as always; counter, signal and staged
    step as in any step. The skip word keeps precedence."""
    h = hyper
    out = dict(p=p.double().clone(), g=g.double().clone(), buf=buf.double().clone(),
               mem={k: v.copy() for k, v in (mem or {}).items()},
               shadow=None if shadow is None else shadow.copy(),
               slot=None if slot is None else slot.double().clone(),
               counter=counter, done=done, signal=signal,
               sched=None if sched is None else dict(sched))
    if counter is not None:
        out["counter"] = counter + int(h.get("delta", 0))
    if signal is not None:
        out["done"], out["signal"] = 0, signal + 1
    if sched is not None and h.get("sched_advance"):
        out["sched"]["next"] = int(sched["step"]) + 1
    if skip:
        return out
    lr = lr_of(h, sched)
    if abs_pass:
        out["p"], out["g"], out["buf"] = out["p"].abs(), out["g"].abs(), out["buf"].abs()
    P, G, B, M = out["p"], out["g"], out["buf"], out["mem"]

    def upd(pv, gv, bv):
        if abs_pass:
            return sgd_abs(pv, gv, bv, lr, h["momentum"], h["wd"], h["grad_scale"], h["nesterov"])
        return sgd_ref(pv, gv, bv, lr, h["momentum"], h["wd"], h["grad_scale"], h["nesterov"],
                       exact=exact)

    def bits(new64, lo, hi):
        if pack_source is not None:
            return bf16_rne_bits(pack_source[lo:hi])
        return bf16_bits_of(new64)

    for it in items:
        kind, a, b_, c = (int(v) for v in it)
        if guard_skipped and kind in (0, 1, 2, 3):
            if not h.get("zero_grad"):
                continue
            if kind == 1:
                d = descs[a]
                TK, TC = tile_dims(int(d[4]) * int(d[5]))
                c1r = max(c, min(int(d[2]), c + TC))
                _master_view(G, d)[b_:min(int(d[1]), b_ + TK), :, :, c:c1r] = 0.0
            else:
                lo = a + (int(descs[c][0]) if kind == 2 else 0)
                G[lo:lo + b_] = 0.0
        elif kind in (0, 3):
            sl = slice(a, a + b_)
            np_, nb = upd(P[sl], G[sl], B[sl])
            P[sl], B[sl] = np_, nb
            if h.get("zero_grad"):
                G[sl] = 0.0
            if kind == 3 and not abs_pass:
                if out["shadow"] is not None:
                    out["shadow"][sl] = bits(np_, a, a + b_)
                if c >= 0 and out["slot"] is not None:
                    out["slot"][c:c + b_] = np_
        elif kind == 4:
            G[a:a + b_] = 0.0
        elif kind in (2, 5):
            d = descs[c]
            lo = int(d[0]) + a
            sl = slice(lo, lo + b_)
            if kind == 2:
                np_, nb = upd(P[sl], G[sl], B[sl])
                P[sl], B[sl] = np_, nb
                if h.get("zero_grad"):
                    G[sl] = 0.0
            if not abs_pass:
                M[int(d[6])][a:a + b_] = bits(P[sl], lo, lo + b_)
        elif kind == 1:
            d = descs[a]
            K, Cr, C, R, S = (int(d[i]) for i in (1, 2, 3, 4, 5))
            TK, TC = tile_dims(R * S)
            k0, c0 = b_, c
            k1 = min(K, k0 + TK)
            c1r = max(c0, min(Cr, c0 + TC))   # real channels of the tile: [c0, c1r)
            c1p = min(C, c0 + TC)             # padded channels of the tile: [c0, c1p)
            pv, gv, bv = (_master_view(t, d)[k0:k1, :, :, c0:c1r] for t in (P, G, B))
            np_, nb = upd(pv, gv, bv)
            pv[...], bv[...] = np_, nb
            if h.get("zero_grad"):
                gv[...] = 0.0
            if abs_pass:
                continue
            if pack_source is not None:
                src = _master_view(torch.from_numpy(pack_source), d)[k0:k1, :, :, c0:c1r]
                nbits = bf16_rne_bits(src.contiguous().numpy())
            else:
                nbits = bf16_bits_of(np_.contiguous())
            if int(d[6]):
                wc = M[int(d[6])][:K * R * S * C].reshape(K, R, S, C)
                wc[k0:k1, :, :, c0:c1r] = nbits
                wc[k0:k1, :, :, c1r:c1p] = 0          # pad channels: +0
            if int(d[7]):
                wt = M[int(d[7])][:C * R * S * K].reshape(C, R, S, K)
                wt[c0:c1r, :, :, k0:k1] = nbits.transpose(3, 1, 2, 0)  # rows c >= Cr: untouched
        else:
            raise ValueError(f"unknown item kind {kind}")
    return out


def tile_items(desc_index, d):
    """Every tile item of descriptor ``d``."""
    K, C, R, S = int(d[1]), int(d[3]), int(d[4]), int(d[5])
    TK, TC = tile_dims(R * S)
    return [[1, desc_index, k0, c0] for k0 in range(0, K, TK) for c0 in range(0, C, TC)]


def shard_tail_ref(segs, src, dst, packs, mem=None, signal=None, skip=0):
    """shard_tail: every segment {src, dst, count, -} copied from ``src`` into ``dst`` (fp32 bit
    copies: numpy float32 arrays), then the Wc of every pack descriptor rebuilt from the complete
    masters (``dst`` is the arena). done is 0 afterwards; the signal is raised, skipped or not; a
    skip leaves dst and every Wc untouched."""
    dst = dst.copy()
    mem = {k: v.copy() for k, v in (mem or {}).items()}
    sig = None if signal is None else signal + 1
    if skip:
        return dst, mem, 0, sig
    du, su = dst.view(np.uint32), src.view(np.uint32)
    for s, d, n, _ in segs:
        du[d:d + n] = su[s:s + n]
    for d in packs:
        pack_ref(dst, d, wc=mem[int(d[6])])
    return dst, mem, 0, sig
