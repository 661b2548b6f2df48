"""RepVGG (Ding et al. 2021, "RepVGG: Making VGG-style ConvNets Great Again"), training form.

A block sums three parallel branches before its ReLU: 3x3 conv + BN (``rbr_dense``), 1x1 conv +
BN (``rbr_1x1``) and, between equal shapes, a BatchNorm of the input (``rbr_identity``). Five
stages, the first block of each with stride 2, global average pool, ``linear``. Module and
state-dict names follow the published model: ``stage0`` (one block), ``stage1..4.<i>``,
``rbr_dense.conv`` / ``.bn``, ``rbr_1x1.conv`` / ``.bn``, ``rbr_identity``, ``linear``; convs
without bias. RepVGG-A0 has 9 108 968 parameters in this form at 1000 classes.

GPU execution: a block is one ``rep_block`` Function: the two convs on the MFMA implicit GEMM,
then csrc/kernels/rep_bn.hip normalises the three inputs and writes the output in one pass; a
block also leaves the statistics of its output for its successor's identity BatchNorm. CPU
execution is plain ATen. ``reparameterize()`` folds a trained model into the deploy form, one 3x3
conv with bias + ReLU per block.
"""
import torch
import torch.nn as nn

# blocks per stage (stage0 first), widths
_VARIANTS = {"repvgg_a0": ((1, 2, 4, 14, 1), (48, 48, 96, 192, 1280)),
             "repvgg_a1": ((1, 2, 4, 14, 1), (64, 64, 128, 256, 1280))}


def _conv_bn(cin, cout, k, stride):
    m = nn.Sequential()
    m.add_module("conv", nn.Conv2d(cin, cout, k, stride, k // 2, bias=False))
    m.add_module("bn", nn.BatchNorm2d(cout))
    return m


class RepVGGBlock(nn.Module):
    def __init__(self, cin, cout, stride=1):
        super().__init__()
        self.rbr_identity = nn.BatchNorm2d(cin) if cin == cout and stride == 1 else None
        self.rbr_dense = _conv_bn(cin, cout, 3, stride)
        self.rbr_1x1 = _conv_bn(cin, cout, 1, stride)
        self._spec = None

    def forward(self, x):  # CPU / ATen path
        y = self.rbr_dense(x) + self.rbr_1x1(x)
        if self.rbr_identity is not None:
            y = y + self.rbr_identity(x)
        return torch.relu(y)

    def spec(self):
        from ..ops.layers import RepBlockSpec
        if self._spec is None:
            d, o = self.rbr_dense, self.rbr_1x1
            cin_pad = 8 if d.conv.in_channels % 8 else None  # the image: 3 channels padded to 8
            self._spec = RepBlockSpec(d.conv, d.bn, o.conv, o.bn, self.rbr_identity,
                                      cin_pad=cin_pad)
        return self._spec

    def forward_fused(self, h, next_block=None):
        from ..ops.layers import rep_block
        return rep_block(h, self.spec(), next_block.spec() if next_block is not None else None)

    def fold(self):
        """(weight, bias) of the one 3x3 conv this block equals in eval mode, in fp32 (or the
        parameters' wider type): each branch's BatchNorm folded into its kernel from the running
        statistics, the 1x1 kernel and the identity placed at the centre tap."""
        def fold_bn(w, bn):
            t = bn.weight / torch.sqrt(bn.running_var + bn.eps)
            return w * t.reshape(-1, 1, 1, 1), bn.bias - bn.running_mean * t
        w3, b3 = fold_bn(self.rbr_dense.conv.weight, self.rbr_dense.bn)
        w1, b1 = fold_bn(self.rbr_1x1.conv.weight, self.rbr_1x1.bn)
        w, b = w3 + nn.functional.pad(w1, [1, 1, 1, 1]), b3 + b1
        if self.rbr_identity is not None:
            eye = torch.eye(w.shape[0], dtype=w.dtype, device=w.device).reshape(*w.shape[:2], 1, 1)
            w0, b0 = fold_bn(nn.functional.pad(eye, [1, 1, 1, 1]), self.rbr_identity)
            w, b = w + w0, b + b0
        return w.detach(), b.detach()


class RepVGG(nn.Module):
    def __init__(self, blocks, widths, num_classes=1000):
        super().__init__()
        self.stage0 = RepVGGBlock(3, widths[0], 2)
        c = widths[0]
        for i in range(1, 5):
            layers = []
            for j in range(blocks[i]):
                layers.append(RepVGGBlock(c, widths[i], 2 if j == 0 else 1))
                c = widths[i]
            setattr(self, f"stage{i}", nn.Sequential(*layers))
        self.linear = nn.Linear(c, num_classes)
        self._fc_spec = None
        self._gpu_ready = False

    def blocks(self):
        return [self.stage0] + [b for i in range(1, 5) for b in getattr(self, f"stage{i}")]

    def _gpu_specs(self):
        from ..ops.layers import LinearGemmSpec
        if not self._gpu_ready:
            for b in self.blocks():
                b.spec()
            # the MFMA GEMM head needs a multiple of 8 outputs; else the small-head kernels
            if self.linear.out_features % 8 == 0:
                self._fc_spec = LinearGemmSpec(self.linear)
            self._gpu_ready = True
        return self._fc_spec

    def fused_plan(self):
        fc = self._gpu_specs()
        out = [s for b in self.blocks() for s in (b.spec().s3, b.spec().s1)]
        return out + ([fc] if fc is not None else [])

    def forward(self, x):
        blocks = self.blocks()
        if not x.is_cuda:
            for b in blocks:
                x = b(x)
            return self.linear(torch.flatten(x.mean((2, 3)), 1))
        from ..ops.common import step_scratch
        from ..ops.layers import global_avg_pool, linear_gemm, linear_small, to_nhwc_input
        fc = self._gpu_specs()
        step_scratch(x.device).zero()
        if self.training:
            self._bump_batches_tracked()
        h = to_nhwc_input(x, 8)
        for b, nxt in zip(blocks, blocks[1:] + [None]):
            h = b.forward_fused(h, nxt)
        h = global_avg_pool(h)
        return linear_gemm(h, fc) if fc is not None else linear_small(h, self.linear)

    def _bump_batches_tracked(self):
        nbt = getattr(self, "_nbt", None)
        if nbt is None:
            nbt = [m.num_batches_tracked for m in self.modules()
                   if isinstance(m, nn.BatchNorm2d) and m.num_batches_tracked is not None]
            self._nbt = nbt
        if nbt:
            torch._foreach_add_(nbt, 1)

    def reparameterize(self):
        """The deploy form: per block one Conv2d(3x3, bias) + ReLU, then the same head."""
        stages = []
        for b in self.blocks():
            w, bias = b.fold()
            conv = nn.Conv2d(w.shape[1], w.shape[0], 3, b.rbr_dense.conv.stride, 1)
            conv.weight.data, conv.bias.data = w.clone(), bias.clone()
            stages.append(nn.Sequential(conv, nn.ReLU()))
        head = nn.Linear(self.linear.in_features, self.linear.out_features)
        head.load_state_dict(self.linear.state_dict())
        return nn.Sequential(*stages, nn.AdaptiveAvgPool2d(1), nn.Flatten(),
                             head.to(self.linear.weight.dtype))


def repvgg(name, num_classes=1000):
    blocks, widths = _VARIANTS[name]
    return RepVGG(blocks, widths, num_classes)
