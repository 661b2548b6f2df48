"""RepVGG blocks (csrc/kernels/rep_bn.hip, ops/layers.py rep_block) on the gfx950 path vs the CPU
fp32 ATen oracle, with the criteria of tests/test_gpu_mobilenet.py."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("stride", [1, 2])
def test_repvgg_block_matches_cpu(native_ext, stride):
    """One block at 4 x 64 x 8 x 8, stride 1 (three branches; the statistics pass over x) and
    stride 2 (two branches): loss within 5 %, cosine > 0.97 on every parameter gradient."""
    from ddp_amd.models.repvgg import RepVGGBlock
    from ddp_amd.optim import FusedSGD
    from ddp_amd.ops.layers import global_avg_pool
    torch.manual_seed(0)
    cpu = RepVGGBlock(64, 64, stride)
    assert (cpu.rbr_identity is not None) == (stride == 1)
    for m in cpu.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.1)
    gpu = copy.deepcopy(cpu).cuda()
    FusedSGD(gpu.parameters(), lr=0.1).zero_grad()
    x = torch.randn(4, 64, 8, 8).to(torch.bfloat16).float()
    w = torch.randn(4, 64)
    out_c = (cpu(x).mean((2, 3)) * w).sum()
    out_c.backward()
    xn = x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).cuda().requires_grad_(True)
    out_g = (global_avg_pool(gpu.forward_fused(xn)).float() * w.cuda()).sum()
    out_g.backward()
    torch.cuda.synchronize()
    out_g, out_c = float(out_g.detach()), float(out_c.detach())
    assert abs(out_g - out_c) < 0.05 * max(1.0, abs(out_c))
    cos = {}
    for (n, pc), pg in zip(cpu.named_parameters(), gpu.parameters()):
        a, b = pg.grad.cpu().reshape(-1), pc.grad.reshape(-1)
        cos[n] = float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-20))
    print(cos)
    assert min(cos.values()) > 0.97, cos
    assert bool(torch.isfinite(xn.grad.float()).all())
    # the running statistics moved as the CPU module's did
    for (n, bc), bg in zip(cpu.named_buffers(), gpu.buffers()):
        if n.endswith(("running_mean", "running_var")):
            assert torch.allclose(bg.cpu(), bc, rtol=2e-2, atol=2e-3), n


def test_small_repvgg_graph_replay_matches_eager_steps(native_ext):
    """A narrow RepVGG (blocks [1, 1, 2, 2, 1], widths 16, 16, 32, 64, 128) at 4 x 64 x 64, lr 0:
    replayed captured steps give the eager steps' loss for the same batch within 2 %."""
    import ddp_amd
    from ddp_amd.models.repvgg import RepVGG
    from ddp_amd.engine import CrossEntropyLoss
    from ddp_amd.engine.step import TrainStep
    from ddp_amd.optim import FusedSGD
    from ddp_amd.data import SyntheticImageNet, DeviceLoader
    dev = torch.device("cuda", 0)
    torch.manual_seed(ddp_amd.SEED)
    loader = DeviceLoader(SyntheticImageNet(True, n=8, size=64), 4, dev, 1, 0, train=True, cpad=8)
    model = RepVGG((1, 1, 2, 2, 1), (16, 16, 32, 64, 128)).to(dev)
    opt = FusedSGD(model.parameters(), lr=0.0, momentum=0.9, weight_decay=1e-4)
    step = TrainStep(model, opt, CrossEntropyLoss(), loader, use_graph=True)
    eager = []
    for _ in range(2):  # one pass over the 2 batches of the dataset
        step.warmup(1)
        eager.append(step.pop_loss())
    step.capture()
    step.pop_loss()
    for i in range(4):  # two more passes, replayed
        step.step()
        v = step.pop_loss()
        assert v == v and abs(v - eager[i % 2]) < 2e-2 * abs(eager[i % 2]), (i, v, eager)
    assert bool(torch.isfinite(opt.arena.data).all())
