"""MobileNet v1 (Howard et al. 2017, "MobileNets: Efficient Convolutional Neural Networks for
Mobile Vision Applications"), with plain ReLU as in the paper.

Stem Conv2d(3, 32, 3, stride 2) + BN + ReLU, thirteen depthwise-separable blocks (depthwise 3x3 +
BN + ReLU, pointwise 1x1 + BN + ReLU), global average pool, Linear(1024, classes): 4 231 976
parameters at 1000 classes. ``width_mult`` scales every channel count (rounded to a multiple
of 8). State-dict keys: ``stem.{0,1}``, ``blocks.<i>.{dw,bn1,pw,bn2}``, ``fc``.

GPU execution: every conv + BN + ReLU is one ConvBNAct Function; the depthwise convs run on the
streaming kernels of csrc/kernels/dwconv.hip, the pointwise ones on the MFMA implicit GEMM. A
depthwise layer takes and offers no BatchNorm-backward fusion, so the specs are not chained.
CPU execution is plain ATen.
"""
import torch
import torch.nn as nn

# (output channels of the pointwise conv, stride of the depthwise conv) per block
_BLOCKS = ((64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 2), (512, 1), (512, 1),
           (512, 1), (512, 1), (512, 1), (1024, 2), (1024, 1))


def _width(c, mult):
    return max(8, int(c * mult + 4) // 8 * 8)


class SeparableBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.dw = nn.Conv2d(cin, cin, 3, stride=stride, padding=1, groups=cin, bias=False)
        self.bn1 = nn.BatchNorm2d(cin)
        self.pw = nn.Conv2d(cin, cout, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self._specs = None

    def forward(self, x):  # CPU / ATen path
        x = torch.relu(self.bn1(self.dw(x)))
        return torch.relu(self.bn2(self.pw(x)))

    def specs(self):
        from ..ops.layers import ConvBNActSpec
        if self._specs is None:
            self._specs = (ConvBNActSpec(self.dw, self.bn1, relu=True),
                           ConvBNActSpec(self.pw, self.bn2, relu=True))
        return self._specs

    def forward_fused(self, h):
        from ..ops.layers import conv_bn_act
        s1, s2 = self.specs()
        return conv_bn_act(conv_bn_act(h, s1), s2)


class MobileNetV1(nn.Module):
    def __init__(self, num_classes=1000, width_mult=1.0):
        super().__init__()
        c = _width(32, width_mult)
        self.stem = nn.Sequential(nn.Conv2d(3, c, 3, stride=2, padding=1, bias=False),
                                  nn.BatchNorm2d(c))
        blocks = []
        for k, s in _BLOCKS:
            k = _width(k, width_mult)
            blocks.append(SeparableBlock(c, k, s))
            c = k
        self.blocks = nn.Sequential(*blocks)
        self.fc = nn.Linear(c, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self._stem = None
        self._fc_spec = None

    def _gpu_specs(self):
        from ..ops.layers import ConvBNActSpec, LinearGemmSpec
        if self._stem is None:
            self._stem = ConvBNActSpec(self.stem[0], self.stem[1], relu=True, cin_pad=8)
            # the MFMA GEMM head needs a multiple of 8 outputs; else the small-head kernels
            if self.fc.out_features % 8 == 0:
                self._fc_spec = LinearGemmSpec(self.fc)
            for b in self.blocks:
                b.specs()
        return self._stem, self._fc_spec

    def fused_plan(self):
        stem, fc = self._gpu_specs()
        out = [stem]
        for b in self.blocks:
            out += list(b.specs())
        return out + ([fc] if fc is not None else [])

    def forward(self, x):
        if not x.is_cuda:
            x = torch.relu(self.stem(x))
            x = self.blocks(x)
            return self.fc(torch.flatten(x.mean((2, 3)), 1))
        from ..ops.common import step_scratch
        from ..ops.layers import (conv_bn_act, global_avg_pool, linear_gemm, linear_small,
                                  to_nhwc_input)
        stem, fc = self._gpu_specs()
        step_scratch(x.device).zero()
        if self.training:
            self._bump_batches_tracked()
        h = conv_bn_act(to_nhwc_input(x, 8), stem)
        for b in self.blocks:
            h = b.forward_fused(h)
        h = global_avg_pool(h)
        return linear_gemm(h, fc) if fc is not None else linear_small(h, self.fc)

    def _bump_batches_tracked(self):
        nbt = getattr(self, "_nbt", None)
        if nbt is None:
            nbt = [m.num_batches_tracked for m in self.modules()
                   if isinstance(m, nn.BatchNorm2d) and m.num_batches_tracked is not None]
            self._nbt = nbt
        if nbt:
            torch._foreach_add_(nbt, 1)


def mobilenet_v1(num_classes=1000, width_mult=1.0):
    return MobileNetV1(num_classes, width_mult)
