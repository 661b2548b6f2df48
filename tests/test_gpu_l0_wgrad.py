"""The VGG input block's weight gradient fused into its BN-backward dz pass (conv_l0.hip
l0_bwd_kernel<2> + l0_wgrad_finish_kernel; ops.layers.L0_WGRAD_FUSE): dz is never stored.

The fused call must build dW from exactly the bf16 dz the unfused call stores, so the reference
is a float64 dW computed from that stored dz and the bf16-valued input, and the yardstick is the
error of the existing path (the WGRAD GEMM on the same dz) against the same reference: both are
fp32 sums of the same products in a different order.

Shapes: the smallest at which each part can go wrong —
  N=2, H=4, W=8     every pixel touches a border; 4 tiles; one block
  N=3, H=W=32       odd N, 192 tiles, a partial last block
  N=72, H=W=32      4608 tiles on 4096 waves: some waves own two tiles (accumulation across the
                    tile loop), 1024 block partials in the finish
"""
import copy
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernels import DEV, _conv_setup

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(2, 4, 8), (3, 32, 32), (72, 32, 32)]
K = 64
EPS = 1e-5
# floor of the dW bound: a few fp32 ulps of the norm (relative L2)
ULP_FLOOR = 4 * 2.0 ** -23


class _block:
    """One forward of the input block (nat.l0_fwd) and its two backward forms on the same
    inputs. Every backward call gets its own dgamma / dbeta and zeroed sums of its own, or the
    sums an earlier call accumulated (``sums``: then the dz pass only)."""

    def __init__(self, nat, N, H, W, bias, nrep=16):
        from ddp_amd.ops.common import ptr, stream_handle
        self.nat, self.N, self.H, self.W = nat, N, H, W
        self.conv, self.spec, self.x, self.xn = _conv_setup(N, 8, H, W, K, 3, 1, 1, Creal=3)
        self.bias = self.conv.bias if bias else None
        self.nrep = nrep
        self.gamma = torch.rand(K, device=DEV) + 0.5
        self.beta = torch.randn(K, device=DEV) * 0.1
        g = self.spec.geom(N, H, W)
        assert nat.l0_ok(g)
        stats = torch.zeros(nrep * 2 * K, device=DEV)
        self.coef = torch.full((6 * K,), float("nan"), device=DEV)
        shp = (N, H // 2, W // 2, K)
        self.y = torch.empty(shp, device=DEV, dtype=torch.bfloat16)
        self.code = torch.empty(shp, device=DEV, dtype=torch.uint8)
        self.zw = torch.empty(shp, device=DEV, dtype=torch.bfloat16)
        nat.l0_fwd(g, ptr(self.xn), ptr(self.spec.wc), ptr(self.bias), EPS, 1, ptr(stats),
                   ptr(self.gamma), ptr(self.beta), ptr(self.coef), ptr(self.y), ptr(self.code),
                   ptr(self.zw), stream_handle())
        self.dy = torch.randn(shp, device=DEV).to(torch.bfloat16)
        torch.cuda.synchronize()
        self.coef_fwd = self.coef.clone()

    def _call(self, dz, sums=None, **kw):
        from ddp_amd.ops.common import ptr, stream_handle, weight_krsc
        self.coef.copy_(self.coef_fwd)
        if sums is not None:  # accumulated by an earlier call: the dz pass only
            kw["sums_ready"] = 1
        else:
            sums = torch.zeros(self.nrep * 2 * K, device=DEV)
        dg, db = torch.zeros(K, device=DEV), torch.zeros(K, device=DEV)
        g = self.spec.geom(self.N, self.H, self.W, weight_krsc(kw.get("dwt")))
        kw.pop("dwt", None)
        rc = self.nat.l0_bwd(g, ptr(self.xn), ptr(self.spec.wc), ptr(self.bias), EPS, 1,
                             ptr(self.coef), ptr(self.dy), ptr(sums), ptr(dz), ptr(dg), ptr(db),
                             ptr(self.code), ptr(self.zw), stream_handle(), **kw)
        torch.cuda.synchronize()
        return {"rc": rc, "k": self.coef[4 * K:].clone(), "dgamma": dg, "dbeta": db, "sums": sums}

    def unfused(self):
        dz = torch.full((self.N, self.H, self.W, K), float("nan"), device=DEV,
                        dtype=torch.bfloat16)
        out = self._call(dz)
        out["dz"] = dz
        return out

    def fused(self, dw, ws=None, sums=None):
        from ddp_amd.ops.common import ptr, workspace
        ws = workspace(self.xn.device) if ws is None else ws
        out = self._call(None, sums, dwt=dw, dw=ptr(dw), ws=ptr(ws), ws_elems=ws.numel())
        out["dw"] = dw
        return out

    def ref64(self, dz):
        """float64 dW [K][3][3][3] from the stored bf16 dz and the bf16-valued input."""
        cols = F.unfold(self.x.double(), 3, padding=1)            # [N][27 = (c, r, s)][H * W]
        d = dz.double().reshape(self.N, self.H * self.W, K)        # [N][H * W][K]
        return torch.einsum("npk,ncp->kc", d, cols).reshape(K, 3, 3, 3)

    def existing(self, dz):
        """The path the fused one replaces: conv_wgrad on the stored dz, as conv_backward calls it."""
        from ddp_amd.ops.layers import conv_backward
        dw = torch.zeros_like(self.conv.weight, memory_format=torch.channels_last)
        conv_backward(self.spec, self.xn, dz, dw, False)
        torch.cuda.synchronize()
        return dw


def _bound(blk, un):
    ref = blk.ref64(un["dz"])
    e_exist = float((blk.existing(un["dz"]).double() - ref).norm() / ref.norm())
    return ref, e_exist, max(2 * e_exist, ULP_FLOOR)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_dw_matches_reference(native_ext, shape, bias):
    """dW of the fused call within 2x the existing path's error against the float64 reference
    built from the unfused call's dz; coef[4..5], dgamma, dbeta bit-identical; no dz written.
    Both calls read the same BN-backward sums (accumulated once by the unfused call: the release
    build adds block partials with float atomics, whose order is not fixed), so their dz is the
    same and every difference is the weight gradient's own.
    Measured on MI355X (relative L2 against float64, existing / fused): 5.2e-8 / 4.8e-8 at N=2,
    1.26e-7 / 9.1e-8 at N=3, 1.93e-7 / 2.25e-7 at N=72; the bound is its 4-ulp floor, 4.8e-7."""
    torch.manual_seed(11)
    N, H, W = shape
    blk = _block(native_ext, N, H, W, bias)
    un = blk.unfused()
    assert not torch.isnan(un["dz"].float()).any()
    ref, e_exist, bound = _bound(blk, un)
    guard = torch.full((N, H, W, K), float("nan"), device=DEV, dtype=torch.bfloat16)
    for layout in (torch.channels_last, torch.contiguous_format):  # [K][R][S][3] and [K][3][R][S]
        fu = blk.fused(torch.zeros_like(blk.conv.weight, memory_format=layout), sums=un["sums"])
        assert fu["rc"] == 0
        e_fused = float((fu["dw"].double() - ref).norm() / ref.norm())
        print(f"l0 wgrad N={N} H={H} W={W} bias={bias} layout={layout}: existing {e_exist:.3e} "
              f"fused {e_fused:.3e} bound {bound:.3e}")
        assert e_fused <= bound, (e_fused, e_exist)
        assert torch.equal(fu["k"], un["k"])
        assert torch.equal(fu["dgamma"], un["dgamma"]) and torch.equal(fu["dbeta"], un["dbeta"])
    assert bool(torch.isnan(guard.float()).all())


@pytest.mark.parametrize("shape", SHAPES)
def test_fused_dw_accumulates(native_ext, shape):
    """dw += gradient: a pre-filled dw ends as prefill + gradient, within the same bound."""
    torch.manual_seed(12)
    N, H, W = shape
    blk = _block(native_ext, N, H, W, True)
    un = blk.unfused()
    ref, e_exist, bound = _bound(blk, un)
    pre = torch.randn_like(blk.conv.weight).contiguous(memory_format=torch.channels_last)
    fu = blk.fused(pre.clone(memory_format=torch.channels_last), sums=un["sums"])
    err = float((fu["dw"].double() - pre.double() - ref).norm() / ref.norm())
    print(f"l0 wgrad accumulate N={N}: existing {e_exist:.3e} fused {err:.3e} bound {bound:.3e}")
    assert err <= bound, (err, bound)


def test_fused_needs_its_workspace(native_ext):
    """A workspace smaller than the block partials: the call reports 1 and launches nothing."""
    torch.manual_seed(13)
    blk = _block(native_ext, 3, 32, 32, True)
    dw = torch.zeros_like(blk.conv.weight, memory_format=torch.channels_last)
    small = torch.zeros(48 * 64 * 28 - 1, device=DEV)  # 192 tiles -> 48 blocks
    out = blk.fused(dw, ws=small)
    assert out["rc"] == 1
    assert float(dw.abs().max()) == 0.0 and float(small.abs().max()) == 0.0
    assert float(out["dgamma"].abs().max()) == 0.0


@pytest.mark.parametrize("registered", [True, False])
def test_sgd_in_fused_finish(native_ext, registered):
    """The fused finish takes a registered SGD step (momentum 0.9, wd 1e-4, lr 0.1): master and
    momentum match the closed form on the stored-gradient result, the bf16 operand copy is
    rewritten with its pad channels untouched, and the gradient never reaches memory.
    Unregistered: nothing is taken and the gradient is stored."""
    nat = native_ext
    torch.manual_seed(14)
    N, H = 8, 32  # (16 l0_sums blocks: one per statistics replica, so two calls agree bitwise)
    blk = _block(nat, N, H, H, True)
    dw_ref = blk.fused(torch.zeros_like(blk.conv.weight, memory_format=torch.channels_last))["dw"]
    lr, mom, wd = 0.1, 0.9, 1e-4
    p = blk.conv.weight.detach().clone().contiguous(memory_format=torch.channels_last)
    buf = (torch.randn_like(p) * 1e-3).contiguous(memory_format=torch.channels_last)
    p0, buf0 = p.clone(), buf.clone()
    wc0 = blk.spec.wc.clone()
    dw = torch.zeros_like(p)
    try:
        if registered:
            nat.sgd_fuse_register(dw.data_ptr(), p.data_ptr(), buf.data_ptr(),
                                  blk.spec.wc.data_ptr(), lr, mom, wd, 1.0, 0, clear=1)
        else:
            nat.sgd_fuse_register(0, clear=1)
        nat.sgd_fuse_begin()
        blk.fused(dw)
        taken = nat.sgd_fuse_taken()
    finally:
        nat.sgd_fuse_register(0, clear=1)
    if not registered:
        assert taken == []
        assert torch.equal(p, p0) and torch.equal(buf, buf0) and torch.equal(blk.spec.wc, wc0)
        assert torch.equal(dw, dw_ref)
        return
    assert taken == [dw.data_ptr()]
    assert float(dw.abs().max()) == 0.0  # the gradient never reached memory
    d = dw_ref + wd * p0
    b_ref = mom * buf0 + d
    p_ref = p0 - lr * b_ref
    assert torch.allclose(buf, b_ref, rtol=1e-5, atol=1e-7)
    assert torch.allclose(p, p_ref, rtol=1e-6, atol=1e-7)
    wc = blk.spec.wc.view(K, 3, 3, 8).float()
    assert torch.equal(wc[..., :3], p.permute(0, 2, 3, 1).to(torch.bfloat16).float())
    assert float(wc[..., 3:].abs().max()) == 0.0  # pad channels stay zero


@pytest.mark.parametrize("batch", [32, 128])
def test_model_gradients_match_unfused(native_ext, batch):
    """VGG-11 forward + backward with L0_WGRAD_FUSE on against two runs with it off: every
    parameter's gradient within the run-to-run noise of the two unfused runs (the criterion of
    test_l0_sums_in_finish_match_separate_pass). Batch 32 takes the input block's sums in the
    conv1 dgrad finish, batch 128 runs l0_sums separately; the fused form must be the one taken."""
    from ddp_amd.models import VGG11
    from ddp_amd.engine import CrossEntropyLoss
    from ddp_amd.optim import FusedSGD
    from ddp_amd.ops import layers
    torch.manual_seed(1)
    a = VGG11().cuda()
    b, c = copy.deepcopy(a), copy.deepcopy(a)
    x = torch.randn(batch, 3, 32, 32, device="cuda")
    y = torch.randint(0, 10, (batch,), device="cuda")
    grads, calls = [], []
    saved = layers.L0_WGRAD_FUSE
    orig = native_ext.l0_bwd

    def spy(*args, **kw):
        r = orig(*args, **kw)
        calls.append((bool(kw.get("dw", 0)), int(kw.get("sums_ready", 0)), r))
        return r
    try:
        native_ext.l0_bwd = spy
        for m, on in ((a, True), (b, False), (c, False)):
            layers.L0_WGRAD_FUSE = on
            opt = FusedSGD(m.parameters(), lr=0.1)
            opt.zero_grad()
            CrossEntropyLoss()(m(x), y).backward()
            torch.cuda.synchronize()
            grads.append([p.grad.clone() for p in m.parameters()])
    finally:
        layers.L0_WGRAD_FUSE = saved
        native_ext.l0_bwd = orig
    assert [f for f, _, _ in calls] == [True, False, False]
    assert not calls[0][2], "the fused form must serve the model's input block"
    assert calls[0][1] == (1 if batch == 32 else 0)

    def cos(u, v):
        return float(torch.dot(u.reshape(-1), v.reshape(-1)) / (u.norm() * v.norm() + 1e-20))

    names = [n for n, _ in a.named_parameters()]
    assert float(grads[0][0].norm()) > 0, names[0]
    for n, ga, gb, gc in zip(names, *grads):
        if float(gb.norm()) < 1e-6:
            continue
        base = cos(gb, gc)
        assert cos(ga, gb) >= min(0.98, base - 0.05), (n, cos(ga, gb), base)


def test_captured_step_takes_layer0_sgd(native_ext):
    """A captured TrainStep at batch 32 with the fused weight gradient: captures, replays three
    times with a finite loss, and the input layer's weight takes its SGD step in the finish."""
    from ddp_amd.models import VGG11
    from ddp_amd.engine import CrossEntropyLoss, TrainStep
    from ddp_amd.optim import FusedSGD
    from ddp_amd.data import SyntheticCIFAR10, DeviceLoader
    from ddp_amd.ops import layers
    assert layers.L0_WGRAD_FUSE in (True, False)
    saved = layers.L0_WGRAD_FUSE
    layers.L0_WGRAD_FUSE = True
    try:
        torch.manual_seed(5)
        m = VGG11().cuda()
        opt = FusedSGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        ld = DeviceLoader(SyntheticCIFAR10(True, n=4 * 32), 32, "cuda", cpad=8)
        st = TrainStep(m, opt, CrossEntropyLoss(), ld)
        assert st.opt_in_bwd
        w0 = next(m.parameters())
        before = w0.detach().clone()
        st.warmup(2)
        st.capture()
        assert st.graph is not None
        for _ in range(3):
            st.step()
        torch.cuda.synchronize()
        taken = opt._fused_in_backward()
    finally:
        layers.L0_WGRAD_FUSE = saved
    i0 = next(i for i, p in enumerate(opt.arena.params) if p is w0)
    assert i0 in taken, (i0, sorted(taken))
    assert bool(torch.isfinite(st.loss_sum))
    assert bool(torch.isfinite(w0).all()) and not torch.equal(w0.detach(), before)


def test_fused_dw_is_bitwise_reproducible(native_ext):
    """Deterministic build: two fused backward calls on the same inputs give bitwise-equal dW."""
    so = os.path.join(REPO, "distributed-data-parallel-ml-training_amd",
                      "_native_det" + __import__("sysconfig").get_config_var("EXT_SUFFIX"))
    if not os.path.exists(so):
        raise RuntimeError(f"deterministic build missing: {so} (run __graft_entry__.build())")
    env = dict(os.environ, DDP_AMD_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "l0_wgrad_probe.py")],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res == {"equal": True, "nonzero": True, "finite": True}, res
