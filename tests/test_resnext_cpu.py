"""ResNeXt-50 32x4d module arithmetic (torchvision's keys and shapes); ResNet-50 unchanged."""
import pytest

from ddp_amd.models import build
from ddp_amd.models.resnet import resnet50, resnext50_32x4d


def _n(m):
    return sum(p.numel() for p in m.parameters())


def test_resnext50_parameters_and_grouped_shapes():
    sd = resnext50_32x4d().state_dict()
    assert _n(resnext50_32x4d()) == 25_028_904
    assert tuple(sd["layer1.0.conv2.weight"].shape) == (128, 4, 3, 3)
    assert tuple(sd["layer4.2.conv2.weight"].shape) == (1024, 32, 3, 3)
    assert tuple(sd["layer4.2.conv3.weight"].shape) == (2048, 1024, 1, 1)


@pytest.mark.parametrize("name", ["resnext50_32x4d", "resnet50_32x4d"])
def test_build_takes_both_spellings(name):
    m = build(name, 10)
    assert m.layer1[0].conv2.groups == 32 and _n(m) == _n(resnext50_32x4d(10))
    ref = resnext50_32x4d(10).state_dict()
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == \
        {k: tuple(v.shape) for k, v in ref.items()}


def test_resnet50_is_what_it_was():
    m = resnet50()
    sd = m.state_dict()
    assert _n(m) == 25_557_032 and len(sd) == 320 and len(list(m.parameters())) == 161
    for k, shape in {"conv1.weight": (64, 3, 7, 7), "layer1.0.conv2.weight": (64, 64, 3, 3),
                     "layer1.0.downsample.0.weight": (256, 64, 1, 1),
                     "layer3.5.conv1.weight": (256, 1024, 1, 1),
                     "layer4.2.conv2.weight": (512, 512, 3, 3),
                     "layer4.0.bn2.running_var": (512,), "fc.weight": (1000, 2048)}.items():
        assert tuple(sd[k].shape) == shape, k
    assert m.layer2[0].conv2.groups == 1 and build("resnet50", 10).fc.out_features == 10
