"""MobileNet v1 module arithmetic: parameter counts, shapes, state-dict keys, build spellings."""
import pytest
import torch

from ddp_amd.models import build
from ddp_amd.models.mobilenet import mobilenet_v1


def _n(m):
    return sum(p.numel() for p in m.parameters())


def test_parameters_shapes_and_keys():
    m = mobilenet_v1()
    sd = m.state_dict()
    assert _n(m) == 4_231_976 and _n(mobilenet_v1(10)) == 3_217_226
    for k, shape in {"stem.0.weight": (32, 3, 3, 3), "stem.1.running_mean": (32,),
                     "blocks.0.dw.weight": (32, 1, 3, 3), "blocks.0.pw.weight": (64, 32, 1, 1),
                     "blocks.12.dw.weight": (1024, 1, 3, 3), "blocks.12.bn1.weight": (1024,),
                     "blocks.12.pw.weight": (1024, 1024, 1, 1), "blocks.12.bn2.bias": (1024,),
                     "fc.weight": (1000, 1024)}.items():
        assert tuple(sd[k].shape) == shape, k
    assert [b.dw.stride[0] for b in m.blocks] == [1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1]
    assert all(b.dw.groups == b.dw.in_channels for b in m.blocks)


@pytest.mark.parametrize("name", ["mobilenet_v1", "mobilenet"])
def test_build_takes_both_spellings_and_num_classes(name):
    assert build(name).fc.out_features == 1000
    m = build(name, 10)
    assert m.fc.out_features == 10 and _n(m) == 3_217_226


def test_width_multiplier_and_cpu_forward():
    m = mobilenet_v1(10, width_mult=0.25)
    assert m.blocks[0].dw.in_channels == 8 and m.fc.in_features == 256
    assert tuple(m(torch.randn(2, 3, 32, 32)).shape) == (2, 10)
