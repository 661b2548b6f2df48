"""SE-ResNet-50 / SE-ResNeXt-50 module arithmetic, state keys, build() names and the CPU gate."""
import pytest
import torch

from ddp_amd.models import build
from ddp_amd.models.resnet import SEGate, resnet50, se_resnet50, se_resnext50_32x4d


_n = lambda m: sum(p.numel() for p in m.parameters())  # noqa: E731


def test_se_parameter_counts_and_state_keys():
    m, plain = se_resnet50(), resnet50()
    assert _n(m) == 28_088_024 == _n(plain) + 2_530_992 and _n(se_resnext50_32x4d()) == 27_559_896
    sd, ref = m.state_dict(), plain.state_dict()
    se = {k: tuple(v.shape) for k, v in sd.items() if ".se." in k}
    assert len(se) == 4 * 16 and se["layer1.0.se.fc1.weight"] == (16, 256)
    assert se["layer4.2.se.fc2.weight"] == (2048, 128) and se["layer3.5.se.fc2.bias"] == (1024,)
    assert {k: tuple(v.shape) for k, v in sd.items() if ".se." not in k} == \
        {k: tuple(v.shape) for k, v in ref.items()}
    names = [k for k, _ in m.layer1[0].named_parameters()]
    assert names.index("se.fc1.weight") == names.index("bn3.bias") + 1  # se sits after bn3


@pytest.mark.parametrize("name,groups", [("se_resnet50", 1), ("resnet50_se", 1),
                                         ("se_resnext50_32x4d", 32), ("resnet50_32x4d_se", 32)])
def test_build_takes_the_four_names_and_group_norm_refuses_them(name, groups):
    m = build(name, 10)
    assert m.layer1[0].conv2.groups == groups and m.layer2[1].se.fc1.out_features == 32
    assert m.fc.out_features == 10
    with pytest.raises(ValueError, match="norm group"):
        build(name, 10, norm="group")


def test_cpu_gate_is_the_formula():
    torch.manual_seed(3)
    g = SEGate(64, 16)
    u = torch.randn(3, 64, 5, 4)
    d = lambda t: t.detach().double()
    m = d(u).mean((2, 3))
    h = (m @ d(g.fc1.weight).T + d(g.fc1.bias)).clamp_min(0)
    s = 1 / (1 + torch.exp(-(h @ d(g.fc2.weight).T + d(g.fc2.bias))))
    assert torch.allclose(g(u).double(), d(u) * s[:, :, None, None], rtol=1e-5, atol=1e-6)
