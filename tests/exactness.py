"""Per-element comparison of a kernel's output with an fp64 reference, in two modes.

A relative l2 norm (``rel_err < 1e-2``) averages a kernel's error over the whole tensor: bf16
output rounding alone gives about 1.7e-3, so one wrong tile row, one dropped tap of a corner pixel
or one lost reduction pixel hides below the threshold (tests/test_exactness_cpu.py measures it).
These helpers look at every element instead.

Exact mode (``assert_exact``): integer-valued bf16 operands. Every product and every partial sum
is then an integer; as long as the sum of the magnitudes stays below 2**24, fp32 accumulation is
exact in ANY order (MFMA, split-K slabs, float atomics, LDS reductions), so an fp32 output must
equal the fp64 reference and a bf16 output must equal ``ref64.to(torch.bfloat16)`` (round to
nearest even on both sides). Use it wherever the arithmetic is sums of products.

Bound mode (``assert_within``): kernels whose arithmetic cannot be made exact (BatchNorm, softmax,
averages). The caller derives a per-element bound from the kernel's code -- 2**-8 |ref| per bf16
rounding on the path plus (fp32 roundings on the path) * 2**-24 * (sum of the terms' magnitudes)
-- and writes the count beside the test. Elements may be excluded only where the fp64 reference
itself cannot decide a branch (a ReLU input within its bound of 0, a pool window whose two
largest values are closer than their bound); the excluded share is capped and is a property of
the reference alone.

Exact-mode comparisons are bitwise: the bit patterns of ``got`` and of the reference converted to
its dtype must agree, so a NaN never matches and a kernel's -0 is a mismatch. An exact zero is
expected as +0: the kernels' accumulators start at +0, and a round-to-nearest sum onto +0 never
gives -0. The fp64 reference need not start from an accumulator (a one-term matrix product
0 * -2 is -0), so its zeros are taken as +0 before the comparison.
"""
import math

import torch

BF16_EPS = 2.0 ** -8   # half a bf16 ulp, relative (8 significand bits, round to nearest even)
FP32_EPS = 2.0 ** -24  # half an fp32 ulp, relative
EXACT_LIMIT = 2 ** 24  # integers below it are exact in fp32


def int_tensor(shape, lo, hi, seed, device="cpu", dtype=torch.float32):
    """Seeded integers in [lo, hi] as floating point values (every one is a bf16 number when
    |lo|, |hi| <= 256). Generated on the CPU so a seed names the same tensor everywhere."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int64)
    return t.to(dtype).to(device)


def gauss_bf16(shape, seed, scale=1.0, shift=0.0, device="cpu"):
    """Seeded Gaussian values rounded to bf16, returned as fp32."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(tuple(shape), generator=g) * scale + shift
    return t.to(torch.bfloat16).float().to(device)


def coords(flat, shape):
    """Flat index -> coordinate tuple of a contiguous tensor of ``shape``."""
    out = []
    for d in reversed(tuple(shape)):
        out.append(int(flat % d))
        flat //= d
    return tuple(reversed(out))


def _fmt(c, names):
    if names is None or len(names) != len(c):
        return str(c)
    return "(" + ", ".join(f"{n}={v}" for n, v in zip(names, c)) + ")"


def mismatches(got, want):
    """Boolean tensor: elements of ``got`` whose bit pattern differs from ``want``'s (same dtype,
    fp32 or bf16)."""
    bits = torch.int32 if got.dtype == torch.float32 else torch.int16
    return got.contiguous().view(bits) != want.contiguous().view(bits)


def assert_exact(got, ref64, absref64, names=None, what="output", show=8, unit=1.0):
    """``got`` (fp32 or bf16, any device) equals the fp64 reference bit for bit.

    ``absref64`` is the same operation on the operands' magnitudes (e.g. conv2d(|x|, |w|, |b|)):
    the precondition ``absref64.max() < 2**24`` guarantees that no partial sum in any order
    leaves the exactly representable integers. On a mismatch the message gives the number of
    wrong elements and the first ``show`` with their coordinates (``names`` labels the axes,
    e.g. ("n", "h", "w", "c") or ("k", "r", "s", "c")), got and want. ``unit``: a power of two
    the reference is an integer multiple of (an integer sum scaled by 2**-k stays exact)."""
    assert ref64.dtype == torch.float64, "the reference must be fp64"
    amax = float(absref64.abs().max()) if absref64.numel() else 0.0
    assert amax < EXACT_LIMIT, (f"{what}: sum of magnitudes {amax:.6g} reaches 2**24, the "
                                f"operands do not make fp32 accumulation exact")
    assert unit > 0 and math.frexp(unit)[0] == 0.5, "unit must be a power of two"
    assert bool((ref64 / unit == (ref64 / unit).round()).all()), \
        f"{what}: the reference is not integer valued"
    assert tuple(got.shape) == tuple(ref64.shape), (what, tuple(got.shape), tuple(ref64.shape))
    assert got.dtype in (torch.float32, torch.bfloat16), got.dtype
    g = got.detach().cpu().contiguous()
    want = (ref64.detach().cpu() + 0.0).to(g.dtype).contiguous()  # (-0 + 0 = +0)
    bad = mismatches(g, want).reshape(-1)
    nbad = int(bad.sum())
    if nbad == 0:
        return
    where = torch.nonzero(bad).reshape(-1)[:show].tolist()
    gf, wf = g.reshape(-1), want.reshape(-1)
    lines = [f"  {_fmt(coords(i, g.shape), names)}: got {float(gf[i])!r} want {float(wf[i])!r}"
             for i in where]
    raise AssertionError(f"{what}: {nbad} of {bad.numel()} elements differ from the exact "
                         f"reference; first {len(where)}:\n" + "\n".join(lines))


def assert_within(got, ref64, bound, names=None, exclude=None, max_excluded=0.005,
                  what="output", show=5):
    """|got - ref64| <= bound element for element; returns the worst |err| / bound.

    ``bound`` is a non-negative fp64 tensor (or scalar) derived from the kernel's code, never from
    its output. ``exclude`` marks elements where the reference cannot decide a branch; it must be
    computed from the reference alone, and its share of the tensor is asserted <= ``max_excluded``
    (0.5 %) before the kernel's output is looked at. Where the bound is 0 the element must be
    equal. A NaN in ``got`` always fails."""
    assert ref64.dtype == torch.float64, "the reference must be fp64"
    assert tuple(got.shape) == tuple(ref64.shape), (what, tuple(got.shape), tuple(ref64.shape))
    r = ref64.detach().cpu()
    b = torch.as_tensor(bound, dtype=torch.float64).detach().cpu().expand_as(r)
    assert bool((b >= 0).all()), f"{what}: negative or NaN bound"
    keep = torch.ones_like(r, dtype=torch.bool)
    if exclude is not None:
        ex = exclude.detach().cpu().expand_as(r)
        share = float(ex.double().mean()) if ex.numel() else 0.0
        assert share <= max_excluded, (f"{what}: {share:.4%} of the elements are undecidable in "
                                       f"the reference (cap {max_excluded:.2%}): choose other "
                                       f"inputs")
        keep = ~ex
    g = got.detach().cpu().double()
    err = (g - r).abs()
    ratio = torch.where(b > 0, err / b.clamp_min(1e-300),
                        torch.where(err == 0, torch.zeros_like(err),
                                    torch.full_like(err, float("inf"))))
    ratio = torch.where(torch.isnan(g) | torch.isnan(ratio), torch.full_like(ratio, float("inf")),
                        ratio)
    ratio = torch.where(keep, ratio, torch.zeros_like(ratio))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst <= 1.0:
        return worst
    flat = ratio.reshape(-1)
    nbad = int((flat > 1.0).sum())
    order = torch.argsort(flat, descending=True)[:show].tolist()
    gf, rf, bf_ = g.reshape(-1), r.reshape(-1), b.reshape(-1)
    lines = [f"  {_fmt(coords(i, r.shape), names)}: got {float(gf[i])!r} want {float(rf[i])!r} "
             f"bound {float(bf_[i]):.3e} |err|/bound {float(flat[i]):.3g}" for i in order]
    raise AssertionError(f"{what}: {nbad} of {flat.numel()} elements outside the bound, worst "
                         f"|err|/bound = {worst:.3g}; worst {len(order)}:\n" + "\n".join(lines))


def dot_bound(ref64, absref64, n, bf16_roundings=1):
    """Bound of an fp32-accumulated sum of n terms whose magnitudes sum to ``absref64``, stored
    after ``bf16_roundings`` roundings to bf16: E = n * 2**-24 * T for the accumulation in any
    order, then each rounding adds 2**-8 of the value it rounds (at most |ref| + E)."""
    e = n * FP32_EPS * absref64.abs()
    return bf16_roundings * BF16_EPS * ref64.abs() + (1.0 + bf16_roundings * BF16_EPS) * e
