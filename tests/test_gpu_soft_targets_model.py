"""Label smoothing and mixup at model level on the GPU: eager == captured steps bit for bit in
the deterministic build (tests/soft_probe.py, a subprocess), the pipelined DDP step against the
single-graph step, VGG-11 forward + backward against the CPU fp32 oracle, and ResNet-50's
1000-way loss head."""
import copy
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, ALPHA = 0.1, 0.4


def test_soft_target_steps_eager_equal_captured(native_ext):
    """VGG-11, batch 8, both flags, 3 steps, K = 1 and K = 2 (accum_steps): masters, momentum,
    bf16 copies and cursor of the eager and the captured TrainStep are torch.equal; the lam each
    micro-batch published is the table's entries 0,1,2 (K = 1) and 0,1 | 2,3 | 4,5 (K = 2)."""
    env = dict(os.environ, DDP_AMD_DETERMINISTIC="1")
    env.pop("DDP_AMD_SGD_IN_BWD", None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "soft_probe.py"), "paths"],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    bad = {k: v for k, v in res.items() if v is not True}
    assert not bad, bad


def test_segmented_ddp_step_with_soft_targets_matches_single_graph(native_ext):
    """SegmentedDDPStep (emulated collective, world 1) against TrainStep with both flags: the
    comparison of test_segmented_ddp_step_matches_single_graph (tests/test_gpu_model.py)."""
    from ddp_amd.models import VGG11
    from ddp_amd.engine import CrossEntropyLoss, TrainStep, SegmentedDDPStep
    from ddp_amd.optim import FusedSGD
    from ddp_amd.data import SyntheticCIFAR10, DeviceLoader
    from ddp_amd.parallel import DistributedDataParallel, RcclCommunicator
    torch.manual_seed(4)
    m = DistributedDataParallel(VGG11().cuda(), RcclCommunicator(0, 1, 0), bucket_cap_mb=256.0,
                                first_bucket_cap_mb=256.0)
    opt = FusedSGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    ld = DeviceLoader(SyntheticCIFAR10(True, n=512), 64, "cuda", mixup_alpha=ALPHA)
    crit = CrossEntropyLoss(label_smoothing=E)
    ts = TrainStep(m, opt, crit, ld)
    ss = SegmentedDDPStep(m, opt, crit, ld, split=4, emulate_gbps=171.0)
    ss.WAIT_TIMEOUT_S = 20.0
    ts.warmup(2)
    torch.cuda.synchronize()
    snap = (m.arena.data.clone(), opt.momentum_buffer.clone(), ld.cursor.clone())

    def run(step, fn):
        m.arena.data.copy_(snap[0]); opt.momentum_buffer.copy_(snap[1]); ld.cursor.copy_(snap[2])
        m.arena.grad.zero_()
        for sp in m.module.fused_plan():
            sp._packed_version = None
            sp.maybe_pack()
        torch.cuda.synchronize()
        fn()
        torch.cuda.synchronize()
        assert int(ld.cursor.item()) == int(snap[2].item()) + 1
        assert step.lams() == [float(ld.lam_table[int(snap[2].item())])]
        return m.arena.data - snap[0]

    def cos(a, b):
        return float(torch.dot(a, b) / (a.norm() * b.norm()))

    ref, ref2 = run(ts, ts._body), run(ts, ts._body)
    base = cos(ref, ref2)  # two executions differ by float-atomic ordering
    seg = run(ss, ss._body)
    ss.warmup(1)
    ss.capture()
    graph = run(ss, ss.step)
    ss.check_error()
    assert float(ref.norm()) > 0
    for d in (seg, graph):
        assert cos(ref, d) > min(0.99, base - 0.005), (cos(ref, d), base)
        assert abs(float(d.norm()) / float(ref.norm()) - 1) < 0.02
    m.close()


def test_vgg11_soft_forward_backward_matches_cpu_oracle(native_ext):
    """One forward + backward of VGG-11 with soft targets (E = 0.1, partners = the labels
    reversed, lam = 0.3) through forward_loss against the CPU fp32 oracles, with the bounds
    test_vgg11_forward_backward_matches_cpu_oracle applies to the plain loss."""
    from test_gpu_model import _emulated_vgg_forward, rel
    from ddp_amd.models import VGG11
    from ddp_amd.ops.common import SoftTarget
    from ddp_amd.optim import FusedSGD
    torch.manual_seed(1)
    cpu = VGG11()
    emu = copy.deepcopy(cpu)
    gpu = copy.deepcopy(cpu).cuda()
    FusedSGD(gpu.parameters(), lr=0.1).zero_grad()
    x = torch.randn(32, 3, 32, 32).to(torch.bfloat16).float()
    y = torch.randint(0, 10, (32,))
    y2, lam = y.flip(0).contiguous(), torch.tensor([0.3])
    soft = SoftTarget(E, y2, lam)
    lc = soft.torch_loss(cpu(x), y)
    lc.backward()
    le = soft.torch_loss(_emulated_vgg_forward(emu, x), y)
    le.backward()
    plain = float(F.cross_entropy(cpu(x), y).detach())
    lg = gpu.forward_loss(x.cuda(), y.cuda(), soft=SoftTarget(E, y2.cuda(), lam.cuda()))
    lg.backward()
    torch.cuda.synchronize()
    assert abs(float(lc) - plain) > 1e-3  # the soft loss is another number than the plain one
    assert abs(float(lg) - float(lc)) < 0.05 * max(1.0, abs(float(lc)))
    assert abs(float(lg) - float(le)) < 1e-2 * max(1.0, abs(float(le)))
    cos, errs = {}, {}
    for (n, pe), pg in zip(emu.named_parameters(), gpu.parameters()):
        g, e = pg.grad.cpu().reshape(-1), pe.grad.reshape(-1)
        if n.startswith("layers.") and n.endswith("bias") and \
                isinstance(emu.layers[int(n.split(".")[1])], torch.nn.Conv2d):
            assert float(g.abs().max()) < 1e-3, n
            continue
        cos[n] = float(torch.dot(g, e) / (g.norm() * e.norm() + 1e-20))
        errs[n] = rel(g, e)
    print("cosine vs bf16-emulated oracle:", {k: round(v, 4) for k, v in cos.items()})
    print("rel err vs bf16-emulated oracle:", {k: round(v, 4) for k, v in errs.items()})
    bad = {k: v for k, v in cos.items() if v < 0.95}
    assert not bad, bad
    for n in ("fc1.weight", "fc1.bias", "layers.26.weight", "layers.26.bias"):
        assert errs[n] < 0.03, (n, errs[n])


def test_resnet_head_soft_loss_against_fp64(native_ext):
    """ResNet-50's loss head alone: [4][1000] bf16 logits through ``cross_entropy`` (the
    criterion's GPU path) with soft targets, loss and gradient per element against fp64 with
    the bounds of tests/test_gpu_soft_targets.py."""
    from exactness import assert_within
    from test_gpu_soft_targets import soft_ce_bounds, torch_soft_loss
    from ddp_amd.engine import CrossEntropyLoss
    B, J, lam = 4, 1000, 0.3
    g = torch.Generator().manual_seed(9)
    logits = (torch.randn(B, J, generator=g) * 3).to(torch.bfloat16)
    ya = torch.tensor([0, J - 1, 17, 500])
    yb = ya.flip(0).contiguous()
    ld = logits.cuda().requires_grad_(True)
    crit = CrossEntropyLoss(label_smoothing=E)
    loss = crit(ld, ya.cuda(), (yb.cuda(), torch.tensor([lam], device="cuda")))
    loss.backward()
    torch.cuda.synchronize()
    l64 = logits.double()
    want, loss_bound, d, d_bound = soft_ce_bounds(l64, ya, yb, E, lam, torch.zeros_like(l64), J, 1)
    assert torch.allclose(want, torch_soft_loss(l64, ya, yb, E, lam), rtol=1e-11, atol=1e-11)
    assert_within(loss.detach().cpu().double().view(1), want.view(1), loss_bound.view(1),
                  what="loss")
    assert ld.grad.dtype == torch.bfloat16
    assert_within(ld.grad, d, d_bound, ("b", "j"), what="dlogits")
    # the same criterion without a partner: label smoothing alone, torch's own formula
    l2 = crit(ld.detach(), ya.cuda())
    want2, bound2, _, _ = soft_ce_bounds(l64, ya, ya, E, 1.0, torch.zeros_like(l64), J, 1)
    assert torch.allclose(want2, F.cross_entropy(
        l64, ya, label_smoothing=float(torch.tensor(E, dtype=torch.float32))), rtol=1e-11, atol=1e-11)
    assert_within(l2.cpu().double().view(1), want2.view(1), bound2.view(1), what="smoothed loss")
