"""RepVGG on the CPU: the published module names, the parameter count, the norm refusals and the
re-parameterisation into the deploy form."""
import pytest
import torch
import torch.nn as nn

from ddp_amd.models import build

WIDTHS, BLOCKS = (48, 48, 96, 192, 1280), (1, 2, 4, 14, 1)


def test_repvgg_a0_names_and_parameter_count():
    m = build("repvgg_a0", num_classes=1000)
    # a plain reconstruction from the widths: per block a 3x3 and a 1x1 conv without bias, two
    # BatchNorms, and a third BatchNorm between equal shapes at stride 1
    want, c = 0, 3
    for width, n in zip(WIDTHS, BLOCKS):
        for j in range(n):
            want += c * width * 10 + 4 * width + (2 * width if c == width and j > 0 else 0)
            c = width
    want += c * 1000 + 1000
    assert sum(p.numel() for p in m.parameters()) == want == 9108968
    keys = set(m.state_dict())
    for k in ("stage0.rbr_dense.conv.weight", "stage0.rbr_1x1.bn.running_var", "linear.bias",
              "stage1.1.rbr_identity.weight", "stage3.13.rbr_1x1.conv.weight",
              "stage4.0.rbr_dense.bn.num_batches_tracked"):
        assert k in keys, k
    assert not any("rbr_identity" in k for k in keys if k.startswith(("stage0.", "stage1.0.",
                                                                      "stage4.0.")))
    assert not any(k.endswith("conv.bias") for k in keys)
    stages = {k.split(".")[0] for k in keys}
    assert stages == {"stage0", "stage1", "stage2", "stage3", "stage4", "linear"}
    assert len(build("repvgg_a1").stage3) == 14 and build("repvgg_a1").linear.in_features == 1280


@pytest.mark.parametrize("norm", ["group", "ghost"])
def test_repvgg_serves_batch_norm_only(norm):
    with pytest.raises(ValueError, match=f"--norm {norm} is served for vgg11/13/16/19"):
        build("repvgg_a0", norm=norm)


def test_reparameterize_equals_three_branch_model():
    torch.manual_seed(3)
    m = build("repvgg_a0", num_classes=16).double()
    for b in m.modules():
        if isinstance(b, nn.BatchNorm2d):
            b.weight.data.uniform_(0.5, 1.5)
            b.bias.data.normal_(0, 0.2)
    m.train()
    for _ in range(3):  # move the running statistics away from (0, 1)
        m(torch.randn(4, 3, 32, 32, dtype=torch.float64))
    m.eval()
    deploy = m.reparameterize().eval()
    x = torch.randn(2, 3, 32, 32, dtype=torch.float64)
    with torch.no_grad():
        want, got = m(x), deploy(x)
    assert float((got - want).abs().max()) <= 1e-9 * float(want.abs().max())
    blocks = [s for s in deploy if isinstance(s, nn.Sequential)]
    assert len(blocks) == sum(BLOCKS)
    for s in blocks:
        convs = [l for l in s.modules() if isinstance(l, nn.Conv2d)]
        assert len(convs) == 1 and convs[0].kernel_size == (3, 3) and convs[0].bias is not None
        assert not any(isinstance(l, nn.BatchNorm2d) for l in s.modules())
