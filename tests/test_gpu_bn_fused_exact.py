"""Exact per-element tests of the BatchNorm work that conv_igemm.hip fuses into DGRAD epilogues
and split-K finishes (tests/bn_fused_ref.py has the reference and says why it can be exact).

Every backward site reads the preceding block's scale, shift, mean and invstd from the table
coef[6][C] the test passes in -- powers of two -- with integer dy, w and z, so dx, the routed
gradient, S1 = sum dy_bn and S2 = sum dy_bn * xhat are exact in any order, and with M a power of
two so are k1, k2 and dz: the kernels must equal the fp64 reference bit for bit. Outputs are
pre-filled with NaN and accumulated-onto buffers (sums, dgamma, dbeta, dw) with small integers, so
an unwritten element, a skipped 16-channel block or ``=`` in place of ``+=`` is a mismatch; a
buffer a path must not write is asserted to keep its pre-fill. No element is excluded anywhere.

Shapes are DGRAD geometry (N, C, H, W, K), 3x3 / stride 1 / pad 1 unless named in SHAPES; C is the
preceding block's channel count, z is [N][2H][2W][C] when pooled, else [N][H][W][C].

Column guards of the C = 8 / C = 16 shapes, read before they were run: the generic epilogue loads
the coefficients under ``cok`` (col < Ng) and z after ``if (!cok || row >= args.Mg) continue``; the
lean epilogue skips a column group with ``if (cbase + j * 16 >= args.Ng) continue`` before its
coefficient loads and reads z only for rows with ro[i] >= 0. Ng % 8 == 0, so a lane's 4 columns
are inside or outside together: neither path reads coef or z past C, and neither refuses the shape.

Launch site -> test (the evidence that the site is taken is in each test's docstring):
  generic epilogue, BNF 1 (pooled) and BNF 2 on 64x64      test_sums_in_unsplit_epilogue
  lean epilogue, BNF 2 on the big tiles (unpooled)         test_sums_in_unsplit_epilogue
  splitk_finish_body<true>, np = 4 and np = 1, dense view  test_sums_in_splitk_finish
  splitk_finish_bnbwd_kernel<RPT, POOL>                    test_whole_bn_backward_in_finish
  conv_bwd_pair_kernel<.., 1>                              test_pair (sd = 1)
  bwd_pair_finish_bnbwd_kernel / bwd_pair_finish_kernel<true>   test_pair (sd, sw >= 2)
  splitk_finish_body<true>, ``code`` branch                test_input_block_sums_in_pair_finish
  splitk_finish_bnfwd_kernel<RPT>                          test_bn_forward_in_finish[_tap_reuse]
"""
import pytest
import torch
import torch.nn.functional as F

from bn_fused_ref import (INVSTDS, MEANS, UNIT, assert_dz_exact, bn_bwd_ref, coef_table, z_tensor)
from exactness import FP32_EPS as u_, assert_exact, assert_within, int_tensor, mismatches
from test_gpu_conv_index_math import SHAPES
from test_gpu_elementwise import EPS, bn_fwd_terms, bn_out_bound
from test_gpu_exact import _case, _check_bwd, _dw_start

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
NHWC = ("n", "h", "w", "c")
FUSE_ROWS = 128  # the shipped row limit of the BN-fused finishes (ddp_conv_bn_fuse_rows)
_BN = {}


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _shape(s):
    """A SHAPES name, or (N, C, H, W, K) of a 3x3 / stride 1 / pad 1 convolution."""
    return SHAPES[s] if isinstance(s, str) else (*s, 3, 1, 1)


def _bn(s, pool, relu, crop=0):
    """The conv case of test_gpu_exact plus the preceding block: integer z, the power-of-two
    coefficient table, the integers the accumulated buffers start from, and the fp64 reference
    (computed once, never modified). ``crop``: z is stored ``crop`` pixels taller and wider than
    the 2H x 2W the pool windows cover (a block whose odd size the pool floors)."""
    key = (s, pool, relu, crop)
    if key in _BN:
        return _BN[key]
    shape = _shape(s)
    N, C, H, W = shape[:4]
    c = _case(shape)
    m = 2 if pool else 1
    Hz, Wz = m * H + crop, m * W + crop
    z = z_tensor(N, C, Hz, Wz, 21)
    coef = coef_table(C, 22)
    dx = c["ref"]["dx"].permute(0, 3, 1, 2)
    # (asserts, on the reference alone, that every intermediate of dz is an fp32 number)
    ref = bn_bwd_ref(dx, z[:, :, :m * H, :m * W].contiguous(), coef, pool, relu)
    b = dict(c=c, shape=shape, pool=pool, relu=relu, Hz=Hz, Wz=Wz, ref=ref,
             zn=_nhwc(z).to(BF16).to(DEV), coef=coef.to(DEV).contiguous(),
             sums0=int_tensor((16, 2, C), -3, 3, 23), dg0=int_tensor((C,), -5, 5, 24),
             db0=int_tensor((C,), -5, 5, 25))
    _BN[key] = b
    return b


def _buffers(b):
    N, C, H, W = b["shape"][:4]
    nan = float("nan")
    return dict(dx=torch.full_like(b["c"]["xn"], nan), sums=b["sums0"].to(DEV),
                dz=torch.full((N, b["Hz"], b["Wz"], C), nan, device=DEV, dtype=BF16),
                dg=b["dg0"].to(DEV), db=b["db0"].to(DEV))


def _tuples(b, o, bna, code=None):
    from ddp_amd.ops.common import ptr
    bn = (ptr(b["zn"]), ptr(b["coef"]), ptr(o["sums"]), int(b["pool"]), int(b["relu"]), b["Hz"],
          b["Wz"]) + (() if code is None else (ptr(code),))
    return bn, ((ptr(o["dz"]), ptr(o["dg"]), ptr(o["db"])) if bna else None)


def _dgrad(nat, b, splits, bna):
    from ddp_amd.ops.common import ptr, stream_handle, workspace
    c = b["c"]
    N, C, H, W = b["shape"][:4]
    ws = workspace(torch.device(DEV))
    o = _buffers(b)
    bn, ba = _tuples(b, o, bna)
    o["done"] = nat.conv_dgrad(c["spec"].geom(N, H, W), ptr(c["dzn"]), ptr(c["spec"].wc),
                               ptr(o["dx"]), ptr(ws), ws.numel(), splits, stream_handle(), bn=bn,
                               bna=ba)
    torch.cuda.synchronize()
    return o


def _same(t, start):
    return not bool(mismatches(t.detach().cpu().contiguous(),
                               start.to(t.dtype).reshape(t.shape).contiguous()).any())


def _all_nan(t):
    return bool(torch.isnan(t.float()).all())


def _check_sums(b, o, what):
    """The 16 replicas summed: pre-fill + S1 | S2, exactly (integers times UNIT = the product of
    the table's smallest powers of two, |mean step| 1/2 * invstd 1/2)."""
    r = b["ref"]
    st = o["sums"].view(16, 2, -1).cpu().double().sum(0).float()
    pre, apre = b["sums0"].double().sum(0), b["sums0"].abs().double().sum(0)
    assert_exact(st[0], pre[0] + r["S1"], apre[0] + r["A1"], ("c",), what + " S1", unit=UNIT)
    assert_exact(st[1], pre[1] + r["S2"], (apre[1] + r["A2"]) / UNIT, ("c",), what + " S2",
                 unit=UNIT)


def _check_plain(b, o, what, bna):
    """The path that stores dx and adds the sums; a BnBwdApply it declined is left untouched."""
    assert not o["done"], what + ": the BN backward must not be reported as fused"
    _check_bwd(b["c"], o["dx"], None, what)
    _check_sums(b, o, what)
    assert _all_nan(o["dz"]) and _same(o["dg"], b["dg0"]) and _same(o["db"], b["db0"]), \
        what + ": dz / dgamma / dbeta written by a finish that did not fuse"


def _check_fused(b, o, what):
    """The finish that runs the whole BN backward: dgamma / dbeta accumulated exactly, dz on all
    four pre-pool pixels of every window; dx and the sums replicas are not written (api.h
    BnBwdApply: "the dgrad output itself is never stored"; the kernel never touches bn.sums)."""
    r = b["ref"]
    assert o["done"], what + ": the finish must take the whole BN backward"
    assert_exact(o["dg"], b["dg0"].double() + r["S2"], (b["dg0"].abs().double() + r["A2"]) / UNIT,
                 ("c",), what + " dgamma", unit=UNIT)
    assert_exact(o["db"], b["db0"].double() + r["S1"], b["db0"].abs().double() + r["A1"], ("c",),
                 what + " dbeta")
    if r["pow2"]:
        # zeros without their sign: dz = sc * inner is -0 for sc < 0, inner = +0 (and sc = 0,
        # inner < 0), which assert_exact's "+0" rule for accumulated sums would reject
        assert_dz_exact(o["dz"], _nhwc(r["dz"]), NHWC, what + " dz")
    else:  # M no power of two: the bound counted beside bn_fused_ref._finish
        assert_within(o["dz"], _nhwc(r["dz"]), _nhwc(r["dz_bound"]), NHWC, what=what + " dz")
    assert _all_nan(o["dx"]), what + ": dx written by the fused finish"
    assert _same(o["sums"], b["sums0"]), what + ": sums replicas written by the fused finish"


# ------------------------------------------------------------------ a. the unsplit epilogue
EPI_CASES = [("corner16", 1), ("pm4x4", 0), ("pm4x4", 1), ("pm4x4_n3", 1), ("odd5x5", 1),
             ("s1_1x1", 1)]


@pytest.mark.parametrize("pool", [1, 0])
@pytest.mark.parametrize("tile", range(8))
@pytest.mark.parametrize("name,rows_pm", EPI_CASES)
def test_sums_in_unsplit_epilogue(native_ext, name, rows_pm, tile, pool):
    """splits = 1, so no finish exists: the GEMM epilogue alone stores dx and adds the sums (the
    generic path when pooled or on the 64x64 tile, the lean path unpooled on the other tiles;
    pm4x4 in NHWC and in pixel-major row order). ReLU on and off."""
    nat = native_ext
    nat.conv_force_tile(tile + 1, 0)
    nat.conv_rows_pm_set(rows_pm)
    try:
        for relu in (1, 0):
            b = _bn(name, pool, relu)
            o = _dgrad(nat, b, 1, False)
            _check_plain(b, o, f"{name} tile {tile} pool {pool} relu {relu} pm {rows_pm}", False)
    finally:
        nat.conv_force_tile(0, 0)
        nat.conv_rows_pm_set(1)


# ------------------------------------------------------------------ b. the plain split-K finish
FINISH_CASES = [(n, p, 1) for n, p in EPI_CASES] + [("dense2x2", 1, 1), ("dense2x2", 1, 0)]


@pytest.mark.parametrize("pool", [1, 0])
@pytest.mark.parametrize("splits", [2, 3])
@pytest.mark.parametrize("name,rows_pm,dense", FINISH_CASES)
def test_sums_in_splitk_finish(native_ext, name, rows_pm, dense, splits, pool):
    """Forced splits on the 64x64 tile: the epilogue writes fp32 slabs only, the finish stores dx
    and adds the sums (splitk_finish_body<true>: np = 4 pooled, np = 1 unpooled; the 2x2 images
    as the dense GEMM's finish view and as the implicit GEMM)."""
    nat = native_ext
    nat.conv_force_tile(4, 0)
    nat.conv_rows_pm_set(rows_pm)
    nat.conv_dense2x2_set(dense)
    try:
        for relu in (1, 0):
            b = _bn(name, pool, relu)
            o = _dgrad(nat, b, splits, False)
            _check_plain(b, o, f"{name} splits {splits} pool {pool} relu {relu}", False)
    finally:
        nat.conv_force_tile(0, 0)
        nat.conv_rows_pm_set(1)
        nat.conv_dense2x2_set(1)


@pytest.mark.parametrize("pool", [1, 0])
@pytest.mark.parametrize("splits", [2, 3])
def test_finish_over_the_row_limit_declines_bn_backward(native_ext, splits, pool):
    """1024 rows with the shipped limit of 128: a BnBwdApply is declined (False), dx and the sums
    come from the plain finish, dz / dgamma / dbeta stay as they were."""
    nat = native_ext
    nat.conv_force_tile(4, 0)
    try:
        b = _bn("pm4x4", pool, 1)
        o = _dgrad(nat, b, splits, True)
    finally:
        nat.conv_force_tile(0, 0)
    _check_plain(b, o, f"pm4x4 over the limit splits {splits} pool {pool}", True)


# ------------------------------------------------------------------ c. the whole BN backward
FUSED_SHAPES = [((8, 64, 4, 4, 64), 1), ((16, 64, 4, 4, 64), 1), ((32, 64, 4, 4, 64), 1),
                ((32, 64, 2, 2, 64), 1), ((32, 64, 2, 2, 64), 0), ((8, 48, 4, 4, 64), 1),
                ((3, 64, 4, 4, 64), 1), ((5, 64, 2, 2, 64), 1)]


@pytest.mark.parametrize("pool", [1, 0])
@pytest.mark.parametrize("splits", [2, 3])
@pytest.mark.parametrize("shape,dense", FUSED_SHAPES)
def test_whole_bn_backward_in_finish(native_ext, shape, dense, splits, pool):
    """splitk_finish_bnbwd_kernel<RPT, POOL> with a 512-row limit: 128 / 256 / 512 rows (RPT 1, 2,
    4), 2x2 images dense and implicit, C = 48 (three 16-channel blocks), Mg = 48 and 20 (idle
    lanes; M no power of two, so dz in bound mode). Returns True."""
    nat = native_ext
    nat.conv_bn_fuse_rows(512)
    nat.conv_dense2x2_set(dense)
    try:
        for relu in (1, 0):
            b = _bn(shape, pool, relu)
            o = _dgrad(nat, b, splits, True)
            _check_fused(b, o, f"{shape} splits {splits} pool {pool} relu {relu} dense {dense}")
    finally:
        nat.conv_bn_fuse_rows(FUSE_ROWS)
        nat.conv_dense2x2_set(1)


@pytest.mark.parametrize("why,pool", [("rows", 1), ("rows", 0), ("channels", 1), ("channels", 0),
                                      ("unsplit", 1), ("unsplit", 0), ("z size", 1)])
def test_whole_bn_backward_refused(native_ext, why, pool):
    """528 rows against the 512-row limit, C = 8 (no 16-channel block), one split (no finish) and
    a pooled z one pixel taller and wider than the windows cover (an unpooled z has the dgrad
    output's size by definition): False, and the plain path's dx
    and sums are right with dz / dgamma / dbeta untouched."""
    nat = native_ext
    shape, splits, crop = {"rows": ((33, 64, 4, 4, 64), 2, 0), "channels": ("odd5x5", 2, 0),
                           "unsplit": ((8, 64, 4, 4, 64), 1, 0),
                           "z size": ((8, 64, 4, 4, 64), 2, 1)}[why]
    nat.conv_bn_fuse_rows(512)
    try:
        b = _bn(shape, pool, 1, crop)
        o = _dgrad(nat, b, splits, True)
    finally:
        nat.conv_bn_fuse_rows(FUSE_ROWS)
    _check_plain(b, o, f"refused ({why}) pool {pool}", True)


# ------------------------------------------------------------------ d. the backward pair
@pytest.mark.parametrize("bna", [False, True])
@pytest.mark.parametrize("sd,sw", [(1, 1), (1, 3), (2, 1), (2, 3), (3, 2)])
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("s", ["corner16", "pm4x4", (16, 64, 4, 4, 64)])
def test_pair(native_ext, s, tile, sd, sw, bna):
    """conv_bwd_pair with forced splits and tile, a 512-row limit, a [K][R][S][C] dw. sd = 1: the
    pair kernel's own epilogue adds the sums (conv_bwd_pair_kernel<.., 1>), return 0. sd >= 2:
    the finish -- grouped with the WGRAD finish when sw >= 2, separate when sw = 1 -- runs the
    whole BN backward when a BnBwdApply is passed and the GEMM has at most 512 rows (return 1:
    corner16 = 512 rows, (16, ..) = 256), else adds the sums (pm4x4 = 1024 rows; no BnBwdApply).
    dw exact in every case."""
    from ddp_amd.ops.common import ptr, stream_handle, weight_krsc, workspace
    nat = native_ext
    nat.conv_bn_fuse_rows(512)
    nat.conv_pair_force(sd, sw, tile)
    try:
        for pool in (1, 0):
            b = _bn(s, pool, 1)
            c = b["c"]
            N, C, H, W = b["shape"][:4]
            ws = workspace(torch.device(DEV))
            o = _buffers(b)
            bn, ba = _tuples(b, o, bna)
            dw = _dw_start(c)
            rc = nat.conv_bwd_pair(c["spec"].geom(N, H, W, weight_krsc(dw)), ptr(c["dzn"]),
                                   ptr(c["spec"].wc), ptr(o["dx"]), ptr(c["xn"]), ptr(dw), ptr(ws),
                                   ws.numel(), stream_handle(), bn=bn, bna=ba)
            torch.cuda.synchronize()
            what = f"{s} pair tile {tile} splits {sd}/{sw} bna {bna} pool {pool}"
            fused = bna and sd >= 2 and N * H * W <= 512
            assert rc == int(fused), (what, rc)
            o["done"] = rc == 1
            _check_bwd(c, None, dw, what)
            if fused:
                _check_fused(b, o, what)
            else:
                _check_plain(b, o, what, bna)
    finally:
        nat.conv_bn_fuse_rows(FUSE_ROWS)
        nat.conv_pair_force(0, 0, 0)


# ------------------------------------------------------------------ e. the input block's sums
def _l0_case(nat):
    """l0_fwd on 2 images gives the input block's code bytes; its zw is replaced by integers and
    rows 2, 3 of its table (all this branch reads) by powers of two. fp64 reference straight from
    the bytes: S1 = sum dx[code < 4], S2 = sum dx (zw - mu) is over the same elements."""
    if "l0" in _BN:
        return _BN["l0"]
    from test_gpu_l0_layout import _decode, _forward
    N = 2
    f = _forward(nat, (N, 32, 32), True)
    c = _case((N, 64, 16, 16, 128, 3, 1, 1))
    g = torch.Generator().manual_seed(31)
    pick = lambda vals: torch.tensor(vals)[torch.randint(0, len(vals), (64,), generator=g)]
    mu, is_ = pick(MEANS), pick(INVSTDS)
    coef = f["coef"].clone().view(6, 64)
    coef[2], coef[3] = mu.to(DEV), is_.to(DEV)
    zw = int_tensor((N, 64, 16, 16), -4, 4, 32).double()
    take = (_decode(f["code"], (N, 32, 32)) < 4).double()
    assert 0.3 < float(take.mean()) < 0.95  # both kinds of window occur
    dxb = c["ref"]["dx"].permute(0, 3, 1, 2).to(BF16).double() * take
    xh = (zw - mu.double().view(1, -1, 1, 1)) * is_.double().view(1, -1, 1, 1)
    sm = lambda v: v.sum((0, 2, 3))
    ref = dict(S1=sm(dxb), S2=sm(dxb * xh), A1=sm(dxb.abs()), A2=sm((dxb * xh).abs()))
    _BN["l0"] = dict(c=c, shape=(N, 64, 16, 16), pool=1, relu=1, Hz=32, Wz=32, ref=ref,
                     zn=_nhwc(zw).to(BF16).to(DEV), coef=coef.reshape(-1).contiguous(),
                     code=f["code"], sums0=int_tensor((16, 2, 64), -3, 3, 23),
                     dg0=int_tensor((64,), -5, 5, 24), db0=int_tensor((64,), -5, 5, 25))
    return _BN["l0"]


def _l0_pair(nat, b, sd, sw, bna, use_ws=True):
    from ddp_amd.ops.common import ptr, stream_handle, weight_krsc, workspace
    c = b["c"]
    ws = workspace(torch.device(DEV))
    o = _buffers(b)
    bn, ba = _tuples(b, o, bna, b["code"])
    dw = _dw_start(c)
    nat.conv_pair_force(sd, sw, 1)
    try:
        rc = nat.conv_bwd_pair(c["spec"].geom(2, 16, 16, weight_krsc(dw)), ptr(c["dzn"]),
                               ptr(c["spec"].wc), ptr(o["dx"]), ptr(c["xn"]), ptr(dw), ptr(ws),
                               ws.numel() if use_ws else 0, stream_handle(), bn=bn, bna=ba)
        torch.cuda.synchronize()
    finally:
        nat.conv_pair_force(0, 0, 0)
    _check_bwd(c, o["dx"], dw, f"l0 pair {sd}/{sw}")
    return rc, o


@pytest.mark.parametrize("sd,sw", [(1, 2), (2, 1), (2, 3), (3, 2)])
def test_input_block_sums_in_pair_finish(native_ext, sd, sw):
    """BnBwdFuse::code: the next layer's pair (N, 64, 16, 16, 128) with a split DGRAD takes the
    input block's sums in its finish and returns 2. A forced sd = 1 is no unsplit DGRAD here:
    ddp_conv_bwd_pair raises the DGRAD split to 2 whenever it is given the code bytes without a
    BnBwdApply ("a split DGRAD costs the pair ~0.5 us where the standalone l0_sums launch it
    replaces costs 3-6 us"), so that case also returns 2 with exact sums."""
    b = _l0_case(native_ext)
    rc, o = _l0_pair(native_ext, b, sd, sw, False)
    assert rc == 2
    o["done"] = False
    _check_sums(b, o, f"l0 sums {sd}/{sw}")


@pytest.mark.parametrize("why", ["no finish", "bna"])
def test_input_block_sums_dropped(native_ext, why):
    """A DGRAD without a split-K finish (no slab workspace: the only way to an unsplit DGRAD, see
    above) and a BnBwdApply, which cannot be served from the code bytes: the pair drops the sums
    (ddp_conv_bwd_pair: "without one, or if the pair would fuse the BN backward into that finish,
    drop them (the caller runs l0_sums)"), returns 0 and leaves sums, dz, dgamma and dbeta
    untouched; dx and dw are still right."""
    b = _l0_case(native_ext)
    rc, o = _l0_pair(native_ext, b, 2, 2, why == "bna", use_ws=why != "no finish")
    assert rc == 0
    assert _same(o["sums"], b["sums0"]) and _all_nan(o["dz"])
    assert _same(o["dg"], b["dg0"]) and _same(o["db"], b["db0"])


def test_dgrad_refuses_code(native_ext):
    """The input block's sums exist in the pair's finish only: conv_dgrad returns -3."""
    from ddp_amd.ops.common import ptr, stream_handle, workspace
    b = _l0_case(native_ext)
    c = b["c"]
    ws = workspace(torch.device(DEV))
    o = _buffers(b)
    bn, _ = _tuples(b, o, False, b["code"])
    with pytest.raises(RuntimeError, match="invalid arguments"):
        native_ext.conv_dgrad(c["spec"].geom(2, 16, 16), ptr(c["dzn"]), ptr(c["spec"].wc),
                              ptr(o["dx"]), ptr(ws), ws.numel(), 2, stream_handle(), bn=bn)
    torch.cuda.synchronize()
    assert _all_nan(o["dx"]) and _same(o["sums"], b["sums0"])


# ------------------------------------------------------------------ f. the BN forward
def _fwd_case(N, C, H, K):
    """Integer x, w, bias; output channel 5 has all-zero weights (constant z, variance 0); gamma
    of mixed sign and exactly 0 on two channels. fp64 references once per shape."""
    key = ("fwd", N, C, H, K)
    if key in _BN:
        return _BN[key]
    from ddp_amd.ops.layers import ConvBNActSpec
    x = int_tensor((N, C, H, H), -1, 1, 41)
    w = int_tensor((K, C, 3, 3), -1, 1, 42)
    w[5] = 0.0
    bias = int_tensor((K,), -3, 3, 43)
    bias[5] = 3.0
    g = torch.Generator().manual_seed(44)
    gamma = (torch.rand(K, generator=g) + 0.5) * (torch.randint(0, 2, (K,), generator=g) * 2 - 1)
    gamma[2] = 0.0
    gamma[K - 3] = 0.0
    assert bool((gamma > 0).any()) and bool((gamma < 0).any())
    beta = torch.randn(K, generator=g) * 0.1
    conv = torch.nn.Conv2d(C, K, 3, 1, 1, bias=True).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(bias)
    spec = ConvBNActSpec(conv, None, cin_pad=C)
    spec.maybe_pack()
    z = F.conv2d(x.double(), w.double(), bias.double(), 1, 1)
    za = F.conv2d(x.abs().double(), w.abs().double(), bias.abs().double(), 1, 1)
    zb = z.to(BF16).double()  # the statistics and the BN input are the ROUNDED conv output
    assert float((zb * zb).sum((0, 2, 3)).max()) < 2 ** 24  # the kernel's fp32 sums are exact
    t = bn_fwd_terms(zb, gamma.float(), beta.float())
    assert bool((zb[:, 5] == 3.0).all())  # the constant channel: variance exactly 0
    _BN[key] = dict(conv=conv, spec=spec, xn=_nhwc(x).to(BF16).to(DEV), z=z, za=za, t=t,
                    gamma=gamma.float().to(DEV), beta=beta.float().to(DEV))
    return _BN[key]


def _check_bn_fwd(f, o, N, H, K, pool, what):
    """z exact; table row 2 (mean) exact for a power-of-two row count; rows 0, 1, 3 and every y
    within the bounds of test_gpu_elementwise.bn_fwd_terms / bn_out_bound, whose table counts
    the same expressions as splitk_finish_bnfwd_kernel's ``if (threadIdx.x < 16)`` block (the
    statistics it folds are exact integer sums below 2**24, for which that table allows one
    rounding each):

    | row | value                | bound                                                       |
    |-----|----------------------|-------------------------------------------------------------|
    | 2   | mu = s1 / M          | dmu = 2u |mu| (exact when M is a power of two)              |
    | 3   | is = rsqrtf(var+eps) | ris |is|  (ris: bn_fwd_terms)                               |
    | 0   | sc = gamma * is      | rsc |sc|, rsc = ris + u                                     |
    | 1   | sh = beta - mu * sc  | rsc |mu sc| + |sc| dmu + (1 + rsc) u (|mu sc| + |sh|): sc's |
    |     |                      | and mu's errors, then the product and the subtraction       |

    Rows 4, 5
    (k1, k2: the backward's) and the statistics replicas are not written by the fused finish
    (splitk_finish_bnfwd_kernel stores rows 0-3 only and has the whole batch in one block: no
    replicas, no atomics), so they keep their pre-fill."""
    t = f["t"]
    assert_exact(o["z"], _nhwc(f["z"]), _nhwc(f["za"]), NHWC, what + " z")
    cf = o["coef"].view(6, K).cpu()
    Mg = N * H * H
    dmu = 2 * u_ * t["mu"].abs()
    if Mg & (Mg - 1) == 0:
        assert _same(cf[2], t["mu"]), what + " mean"
    else:
        assert_within(cf[2], t["mu"], dmu, ("k",), what=what + " mean")
    musc = (t["mu"] * t["sc"]).abs()
    dsh = musc * t["rsc"] + t["sc"].abs() * dmu + (1 + t["rsc"]) * u_ * (musc + t["sh"].abs())
    assert_within(cf[0], t["sc"], t["sc"].abs() * t["rsc"], ("k",), what=what + " scale")
    assert_within(cf[1], t["sh"], dsh, ("k",), what=what + " shift")
    assert_within(cf[3], t["is_"], t["is_"] * t["ris"], ("k",), what=what + " invstd")
    assert bool(torch.isnan(cf[4:]).all()), what + ": table rows 4, 5 written"
    assert _same(o["stats"], o["stats0"]), what + ": statistics replicas written"
    out, bound = bn_out_bound(t, 1, pool)
    assert_within(o["y"], _nhwc(out), _nhwc(bound), NHWC, what=what + " y")  # nothing excluded


def _fwd_buffers(N, H, K, pool):
    Ho = H // 2 if pool else H
    nan = float("nan")
    stats0 = int_tensor((16 * 2 * K,), -3, 3, 45)
    return dict(z=torch.full((N, H, H, K), nan, device=DEV, dtype=BF16),
                y=torch.full((N, Ho, Ho, K), nan, device=DEV, dtype=BF16),
                coef=torch.full((6 * K,), nan, device=DEV), stats0=stats0, stats=stats0.to(DEV))


@pytest.mark.parametrize("pool", [1, 0])
@pytest.mark.parametrize("N,C,H,K", [(8, 64, 4, 64), (16, 64, 4, 64), (32, 64, 4, 64),
                                     (64, 64, 4, 64), (5, 64, 2, 64), (10, 64, 4, 64)])
def test_bn_forward_in_finish(native_ext, N, C, H, K, pool):
    """splitk_finish_bnfwd_kernel<RPT> through conv_fwd_bn with a forced split-K and a 1024-row
    limit: 128 / 256 / 512 / 1024 rows (RPT 1, 2, 4, 8), 20 and 160 rows (partial lane rows).
    Returns True."""
    from ddp_amd.ops.common import load_conv_tuning, ptr, stream_handle, workspace
    nat = native_ext
    f = _fwd_case(N, C, H, K)
    o = _fwd_buffers(N, H, K, pool)
    ws = workspace(torch.device(DEV))
    nat.conv_tune_set(0, N * H * H, K, 9 * C, 3, 4, 2)  # split-K 4 on 64x64 tiles
    nat.conv_bn_fuse_rows(1024)
    try:
        fused = nat.conv_fwd_bn(f["spec"].geom(N, H, H), ptr(f["xn"]), ptr(f["spec"].wc),
                                ptr(f["conv"].bias), ptr(o["z"]), ptr(o["stats"]), ptr(ws),
                                ws.numel(), stream_handle(),
                                (ptr(f["gamma"]), ptr(f["beta"]), EPS, 1, int(pool), ptr(o["coef"]),
                                 ptr(o["y"]), H, H))
        torch.cuda.synchronize()
    finally:
        load_conv_tuning(nat)  # back to the shipped table
        nat.conv_bn_fuse_rows(FUSE_ROWS)
    assert fused, "the split-K GEMM must take the fused BatchNorm finish"
    _check_bn_fwd(f, o, N, H, K, pool, f"bn fwd {(N, C, H, K)} pool {pool}")


@pytest.mark.parametrize("N,C,H,K,pool", [(32, 512, 2, 512, 0), (32, 256, 4, 512, 1)])
def test_bn_forward_in_finish_tap_reuse(native_ext, N, C, H, K, pool):
    """The same finish behind the tap-reuse forward's slabs (conv_fwd_tr returns 2)."""
    from ddp_amd.ops.common import ptr, stream_handle, workspace
    nat = native_ext
    f = _fwd_case(N, C, H, K)
    o = _fwd_buffers(N, H, K, pool)
    ws = workspace(torch.device(DEV))
    nat.conv_tr_set(3, 0, 0, 0, 0, 64, 64, 4, 0)
    nat.conv_bn_fuse_rows(1024)
    try:
        r = nat.conv_fwd_tr(f["spec"].geom(N, H, H), ptr(f["xn"]), ptr(f["spec"].wc),
                            ptr(f["conv"].bias), ptr(o["z"]), ptr(o["stats"]), ptr(ws), ws.numel(),
                            stream_handle(),
                            (ptr(f["gamma"]), ptr(f["beta"]), EPS, 1, int(pool), ptr(o["coef"]),
                             ptr(o["y"]), H, H))
        torch.cuda.synchronize()
    finally:
        nat.conv_tr_set(3, 0, 0, 0, 0, 0, 0, 0, 0)
        nat.conv_bn_fuse_rows(FUSE_ROWS)
    assert r == 2, "the split-K tap-reuse GEMM must take the BatchNorm-fused finish"
    _check_bn_fwd(f, o, N, H, K, pool, f"bn fwd tap reuse {(N, C, H, K)} pool {pool}")
