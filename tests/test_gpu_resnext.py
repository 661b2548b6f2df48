"""ResNeXt (grouped conv2, csrc/kernels/conv_group.hip) on the gfx950 path vs the CPU fp32 ATen
oracle, with the criteria of tests/test_gpu_resnet.py."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("stride", [1, 2])
def test_resnext_bottleneck_matches_cpu(native_ext, stride):
    """Bottleneck(groups=32, base_width=4), identity and stride-2 projection shortcut: loss within
    5 %, cosine > 0.97 on every parameter gradient (test_bottleneck_block_matches_cpu's)."""
    from ddp_amd.models.resnet import Bottleneck
    from ddp_amd.optim import FusedSGD
    from ddp_amd.ops.layers import global_avg_pool
    torch.manual_seed(0)
    ds = None
    if stride == 2:
        ds = torch.nn.Sequential(torch.nn.Conv2d(256, 256, 1, stride=2, bias=False),
                                 torch.nn.BatchNorm2d(256))
    cpu = Bottleneck(256, 64, stride=stride, downsample=ds, groups=32, base_width=4)
    assert tuple(cpu.conv2.weight.shape) == (128, 4, 3, 3)
    gpu = copy.deepcopy(cpu).cuda()
    FusedSGD(gpu.parameters(), lr=0.1).zero_grad()
    x = torch.randn(4, 256, 8, 8).to(torch.bfloat16).float()
    w = torch.randn(4, 256)
    out_c = (cpu(x).mean((2, 3)) * w).sum()
    out_c.backward()
    xn = x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).cuda()
    out_g = (global_avg_pool(gpu.forward_fused(xn)).float() * w.cuda()).sum()
    out_g.backward()
    torch.cuda.synchronize()
    assert abs(float(out_g) - float(out_c)) < 0.05 * max(1.0, abs(float(out_c)))
    cos = {}
    for (n, pc), pg in zip(cpu.named_parameters(), gpu.parameters()):
        a, b = pg.grad.cpu().reshape(-1), pc.grad.reshape(-1)
        cos[n] = float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-20))
    print(cos)
    assert min(cos.values()) > 0.97, cos


def test_small_resnext_graph_replay_matches_eager_steps(native_ext):
    """ResNet(layers=(1, 1, 1, 1), groups=32, width_per_group=4) at 4 x 64 x 64, lr 0: replayed
    captured steps give the eager steps' loss for the same batch, within
    test_resnet50_graph_replay_matches_eager_steps' 2 %."""
    import ddp_amd
    from ddp_amd.models.resnet import ResNet
    from ddp_amd.engine import CrossEntropyLoss
    from ddp_amd.engine.step import TrainStep
    from ddp_amd.optim import FusedSGD
    from ddp_amd.data import SyntheticImageNet, DeviceLoader
    dev = torch.device("cuda", 0)
    torch.manual_seed(ddp_amd.SEED)
    loader = DeviceLoader(SyntheticImageNet(True, n=8, size=64), 4, dev, 1, 0, train=True, cpad=8)
    model = ResNet((1, 1, 1, 1), groups=32, width_per_group=4).to(dev)
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


def test_cg2_is_refused(native_ext):
    from ddp_amd.ops.layers import ConvBNActSpec
    conv = torch.nn.Conv2d(64, 64, 3, 1, 1, groups=32, bias=False).cuda()
    with pytest.raises(ValueError, match="channels per group"):
        ConvBNActSpec(conv, torch.nn.BatchNorm2d(64).cuda())
