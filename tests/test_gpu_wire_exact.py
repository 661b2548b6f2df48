"""The gradient-wire and layout kernels (csrc/kernels/comm_util.hip, nchw_to_nhwc of data.hip),
bit for bit against plain references, with the guard bands of tests/test_gpu_update_exact.py: every
buffer is compared whole, so a store one element past a tail or a grid-stride loop that runs
short shows as a coordinate.

Roundings: unpack_bf16, seg_copy_f32, copy_bytes, fill_bytes move bits (none). pack_bf16 and
nchw_to_nhwc round once, to nearest even (update_oracle.bf16_rne_bits). mean_ws adds integers
(exact) and multiplies by fp32(1 / ws): one rounding, and the fp64 product of two fp32 numbers is
exact, so fp32(sum * fp64(fp32(1 / ws))) has that one rounding too. scale and comm_standin are one
fp32 multiplication: fp32(x64 * s64).
"""
import numpy as np
import pytest
import torch

import update_oracle as uo
from exactness import int_tensor
from test_gpu_update_exact import BIG, DEV, GUARD, Buf, bf16_of, same_bits, stream

pytestmark = pytest.mark.gpu

BIG_MEAN = 4096 * 256 + 259            # past the 4096-block cap at one element per thread
BIG_BYTES = (16 << 20) + 16 * 300 + 7  # past the cap at 16 bytes per thread
SIZES = (1, 3, 4, 5, 1023, BIG)


def f32_from_bits(u):
    return torch.from_numpy(np.ascontiguousarray(u).view(np.int32).copy()).view(torch.float32)


def tiled(pat, n):
    return np.resize(pat, n)


# ---------------------------------------------------------------------------------- bf16 wire
@pytest.mark.parametrize("n", [1 << 16, 1, 2, 3, 5, 7])
def test_unpack_bf16_every_pattern(native_ext, n):
    """All 65536 bit patterns (NaN payloads included) widen to pattern << 16; short counts for
    the scalar tail."""
    pat = (np.arange(n, dtype=np.uint32) if n > 7 else
           np.array([0x7fb1, 0x8001, 0x3f80, 0xffff, 0x0080, 0x7f7f, 0xc2ff][:n], dtype=np.uint32))
    y = Buf(n, torch.bfloat16, fill=bf16_of(pat.astype(np.uint16)))
    x = Buf(n)
    yb, xb = y.host(), x.host()
    native_ext.unpack_bf16(y.ptr, n, x.ptr, stream())
    torch.cuda.synchronize()
    same_bits(x.host(), x.expect(xb, f32_from_bits(pat << 16)), "unpacked fp32")
    same_bits(y.host(), yb, "bf16 source")


@pytest.mark.parametrize("n", SIZES)
def test_pack_bf16_patterns(native_ext, n):
    """Zeros, normals and inf must equal the integer round-to-nearest-even formula bitwise; a NaN
    gives a NaN (payload not compared)."""
    u, _ = uo.wire_patterns()
    pat = tiled(u, n)
    if n > len(u):   # beyond the list: seeded random normals
        rng = np.random.RandomState(n % 1000)
        extra = rng.randint(0x00800000, 0x7f800000, n - len(u)).astype(np.uint32)
        pat[len(u):] = extra | (rng.randint(0, 2, n - len(u)).astype(np.uint32) << 31)
    x = Buf(n, fill=f32_from_bits(pat))
    y = Buf(n, torch.bfloat16)
    xb, yb = x.host(), y.host()
    native_ext.pack_bf16(x.ptr, n, y.ptr, stream())
    torch.cuda.synchronize()
    want = uo.bf16_rne_bits(pat.view(np.float32))
    got_full = y.host()
    got = uo.bf16_to_bits(got_full[GUARD:GUARD + n])
    nan = np.isnan(pat.view(np.float32))
    assert (((got[nan] & 0x7f80) == 0x7f80) & ((got[nan] & 0x7f) != 0)).all(), "NaN in, NaN out"
    want[nan] = got[nan]
    same_bits(got_full, y.expect(yb, bf16_of(want)), "packed bf16")
    same_bits(x.host(), xb, "fp32 source")


def test_pack_bf16_subnormals(native_ext, capsys):
    """fp32 subnormal inputs: the conversion may keep them (round to nearest even) or flush them
    to a zero of the input's sign; anything else fails. Prints which was seen."""
    _, s = uo.wire_patterns()
    n = len(s)
    x = Buf(n, fill=f32_from_bits(s))
    y = Buf(n, torch.bfloat16)
    yb = y.host()
    native_ext.pack_bf16(x.ptr, n, y.ptr, stream())
    torch.cuda.synchronize()
    got_full = y.host()
    got = uo.bf16_to_bits(got_full[GUARD:GUARD + n])
    rne = uo.bf16_rne_bits(s.view(np.float32))
    zero = ((s >> 16) & 0x8000).astype(np.uint16)
    is_rne, is_zero = got == rne, got == zero
    decides = rne != zero   # inputs on which the two behaviours differ
    seen = ("round to nearest even (subnormals kept)" if is_rne.all() else
            "flushed to signed zero" if is_zero.all() else "mixed")
    with capsys.disabled():
        print(f"\npack_bf16 on {n} fp32 subnormals ({int(decides.sum())} deciding): {seen}; "
              f"RNE on {int((is_rne & decides).sum())}, signed zero on "
              f"{int((is_zero & decides).sum())} of the deciding inputs")
    want = np.where(is_rne | is_zero, got, rne)
    same_bits(got_full, y.expect(yb, bf16_of(want)), "subnormal in: neither RNE nor a signed zero")


def test_pack_unpack_misaligned_raise(native_ext):
    x, y = Buf(64), Buf(64, torch.bfloat16)
    xb, yb = x.host(), y.host()
    for fn, a, b in ((native_ext.pack_bf16, x.ptr + 4, y.ptr),
                     (native_ext.pack_bf16, x.ptr, y.ptr + 2),
                     (native_ext.unpack_bf16, y.ptr + 2, x.ptr),
                     (native_ext.unpack_bf16, y.ptr, x.ptr + 4)):
        with pytest.raises(RuntimeError):
            fn(a, 8, b, stream())
    torch.cuda.synchronize()
    same_bits(x.host(), xb, "x after the refused calls")
    same_bits(y.host(), yb, "y after the refused calls")


# ------------------------------------------------------------------------------ mean / scale
@pytest.mark.parametrize("n", [1, 255, 257, BIG_MEAN])
@pytest.mark.parametrize("ws", [1, 2, 3, 8])
def test_mean_ws(native_ext, ws, n):
    src = int_tensor((ws, n), -64, 64, 7 * ws + n % 11)
    a, out = Buf(ws * n, fill=src), Buf(n)
    ab, ob = a.host(), out.host()
    native_ext.mean_ws(a.ptr, n, ws, out.ptr, stream())
    torch.cuda.synchronize()
    inv = float(np.float32(1.0) / np.float32(ws))
    want = (src.double().sum(0) * inv).float()   # one rounding: the fp64 product is exact
    same_bits(out.host(), out.expect(ob, want), f"mean over {ws}")
    same_bits(a.host(), ab, "gathered input")


@pytest.mark.parametrize("n", [1, 255, 257, BIG_MEAN])
@pytest.mark.parametrize("s", [0.5, 1.0 / 3.0, 1.0])
def test_scale(native_ext, s, n):
    v = torch.randn(n, generator=torch.Generator().manual_seed(n % 13))
    x = Buf(n, fill=v)
    xb = x.host()
    native_ext.scale(x.ptr, n, s, stream())
    torch.cuda.synchronize()
    want = (v.double() * uo.f32(s)).float()
    same_bits(x.host(), x.expect(xb, want), f"x * {s}")


@pytest.mark.parametrize("passes", [1, 3])
def test_comm_standin_doubles(native_ext, passes):
    """The stand-in collective other tests rely on: scale 2.0 doubles every element once, however
    many paced passes it makes (4 blocks, 50 us, n = 4 * 1000 + 3)."""
    n = 4 * 1000 + 3
    v = torch.randn(n, generator=torch.Generator().manual_seed(5))
    x = Buf(n, fill=v)
    xb = x.host()
    native_ext.comm_standin(x.ptr, n, 4, 50.0, 2.0, stream(), passes=passes)
    torch.cuda.synchronize()
    same_bits(x.host(), x.expect(xb, (v.double() * 2.0).float()), "x * 2")


# ------------------------------------------------------------------------------------- copies
def test_seg_copy_f32(native_ext):
    counts = (0, 1, 255, 256, 257, 1000)
    rng = np.random.RandomState(17)
    src = Buf(1400, fill=f32_from_bits(rng.randint(0, 1 << 32, 1400, dtype=np.uint64)
                                       .astype(np.uint32)))
    dst = Buf(2048)
    table, d = [], 5
    for j, c in enumerate(counts):
        table.append([61 * j, d, c, 0])   # sources overlap: 61 * j + c > 61 * (j + 1)
        d += c + 2
    t = torch.tensor(table, dtype=torch.int32, device=DEV)
    sb, db = src.host(), dst.host()
    native_ext.seg_copy_f32(t.data_ptr(), len(table), src.ptr, dst.ptr, stream())
    native_ext.seg_copy_f32(t.data_ptr(), 0, src.ptr, dst.ptr, stream())   # n = 0: no launch
    torch.cuda.synchronize()
    want = db[GUARD:GUARD + dst.n].clone()
    for s, d, c, _ in table:
        want[d:d + c] = sb[GUARD + s:GUARD + s + c]
    same_bits(dst.host(), dst.expect(db, want), "segments")
    same_bits(src.host(), sb, "source")


def _bytes(n, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8))


def test_copy_and_fill_bytes_offsets(native_ext):
    """dst and src 0, 1, 8, 15 bytes off a 16-byte boundary (the vector path needs both on it),
    n in {1, 15, 16, 17, 4097}; fill values 0, 0x7F, 0xFF."""
    span = 4097 + 16
    for n in (1, 15, 16, 17, 4097):
        data = _bytes(span, n)
        for do in (0, 1, 8, 15):
            for so in (0, 1, 8, 15):
                dst, src = Buf(span, torch.uint8), Buf(span, torch.uint8, fill=data)
                assert dst.ptr % 16 == 0 and src.ptr % 16 == 0
                db, sb = dst.host(), src.host()
                native_ext.copy_bytes(dst.ptr + do, src.ptr + so, n, stream())
                torch.cuda.synchronize()
                want = db.clone()
                want[GUARD + do:GUARD + do + n] = data[so:so + n]
                same_bits(dst.host(), want, f"copy n={n} dst+{do} src+{so}")
                same_bits(src.host(), sb, "copy source")
            v = {0: 0, 1: 0x7F, 8: 0xFF, 15: 0x7F}[do]
            dst = Buf(span, torch.uint8)
            db = dst.host()
            native_ext.fill_bytes(dst.ptr + do, v, n, stream())
            torch.cuda.synchronize()
            want = db.clone()
            want[GUARD + do:GUARD + do + n] = v
            same_bits(dst.host(), want, f"fill n={n} dst+{do} value {v}")


def test_copy_and_fill_bytes_noops(native_ext):
    b = Buf(256, torch.uint8, fill=_bytes(256, 3))
    bb = b.host()
    native_ext.copy_bytes(b.ptr, b.ptr + 64, 0, stream())   # n = 0
    native_ext.copy_bytes(b.ptr + 3, b.ptr + 3, 100, stream())  # dst == src
    native_ext.fill_bytes(b.ptr, 0xFF, 0, stream())
    torch.cuda.synchronize()
    same_bits(b.host(), bb, "no-op calls")


def test_copy_bytes_grid_stride(native_ext):
    n = BIG_BYTES
    data = _bytes(n, 4)
    dst, src = Buf(n, torch.uint8), Buf(n, torch.uint8, fill=data)
    db = dst.host()
    native_ext.copy_bytes(dst.ptr, src.ptr, n, stream())
    torch.cuda.synchronize()
    same_bits(dst.host(), dst.expect(db, data), "16 MiB copy")


def test_fill_bytes_grid_stride(native_ext):
    n = BIG_BYTES
    dst = Buf(n, torch.uint8)
    db = dst.host()
    native_ext.fill_bytes(dst.ptr, 0x7F, n, stream())
    torch.cuda.synchronize()
    same_bits(dst.host(), dst.expect(db, torch.full((n,), 0x7F, dtype=torch.uint8)), "16 MiB fill")


# -------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("N,C,H,W,Cp", [(2, 3, 5, 7, 8), (1, 8, 4, 4, 8), (3, 5, 3, 2, 16)])
def test_nchw_to_nhwc(native_ext, N, C, H, W, Cp):
    """fp32 NCHW -> bf16 NHWC with the channels padded to Cp: round to nearest even, pad channels
    0x0000. Values: the conversion pattern set (zeros, normals, inf) and Gaussians."""
    u, _ = uo.wire_patterns()
    u = u[~np.isnan(u.view(np.float32))]
    n = N * C * H * W
    vals = torch.randn(n, generator=torch.Generator().manual_seed(n))
    k = min(n // 2, len(u))
    vals[:k] = f32_from_bits(np.random.RandomState(n).permutation(u)[:k])
    x = Buf(n, fill=vals)
    out = Buf(N * H * W * Cp, torch.bfloat16)
    xb, ob = x.host(), out.host()
    native_ext.nchw_to_nhwc(x.ptr, N, C, H, W, Cp, out.ptr, stream())
    torch.cuda.synchronize()
    want = np.zeros((N, H, W, Cp), np.uint16)
    want[..., :C] = uo.bf16_rne_bits(vals.view(N, C, H, W).permute(0, 2, 3, 1).contiguous().numpy())
    same_bits(out.host(), out.expect(ob, bf16_of(want.reshape(-1))), "NHWC bf16", (N, H, W, Cp),
              ("n", "h", "w", "c"))
    same_bits(x.host(), xb, "NCHW source")
