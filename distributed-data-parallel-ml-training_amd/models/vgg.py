"""VGG family (VGG-11/13/16/19) for 3x32x32 inputs; 10 classes by default (``num_classes``:
up to 128 on the GPU, e.g. 100 for CIFAR-100).

Reference parity: part1/model.py:3-50 (identical copies in part2/part2a, part2/part2b, part3).
The module tree — ``layers`` (nn.Sequential of Conv2d(3x3,s1,p1,bias) / BatchNorm2d(
track_running_stats=False) / ReLU(inplace) / MaxPool2d(2,2)) and ``fc1`` (Linear(512, classes)) —
is kept exactly so that ``state_dict`` keys and shapes match the reference checkpoint layout
(``layers.{0,4,8,...}.{weight,bias}``, BN without running buffers, ``fc1.{weight,bias}``).

Execution:
* CPU tensors run the ATen modules unchanged (the numerical oracle, and the part1 CPU path).
* GPU tensors run the fused gfx950 path: each Conv->BN->ReLU(->MaxPool) group becomes one
  ``ConvBNAct`` autograd Function (ops/layers.py), activations stay NHWC bf16, the head is a
  fused Linear + loss kernel (one wave per row up to 16 classes, the MFMA head up to 128). Inputs may be NCHW fp32 (converted on device) or the NHWC bf16
  batches produced by the on-device data pipeline (data/loader.py).
"""
import torch
import torch.nn as nn

_cfg = {
    'VGG11': [64, 'M', 128, 'M', 256, 256, 'M', 512, 512, 'M', 512, 512, 'M'],
    'VGG13': [64, 64, 'M', 128, 128, 'M', 256, 256, 'M', 512, 512, 'M', 512, 512, 'M'],
    'VGG16': [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M'],
    'VGG19': [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 256, 'M', 512, 512, 512, 512, 'M',
              512, 512, 512, 512, 'M'],
}

IN_CHANNELS_PADDED = 8  # first conv consumes 3 real + 5 zero channels on the MFMA path


class GhostBatchNorm2d(nn.BatchNorm2d):
    """BatchNorm over fixed-size groups of ``ghost_batch`` images (Hoffer et al. 2017), without
    running statistics. The groups are interleaved as the sharded sampler deals the samples:
    with ngroups = ceil(N / ghost_batch), image n belongs to group n % ngroups, so the sets of
    images that share statistics are the same for every world size that divides N / ghost_batch.
    Parameter names and shapes are BatchNorm2d's; one group is the plain BatchNorm call. This
    forward is the CPU path (and the oracle); GPU tensors run csrc/kernels/ghost_bn.hip."""

    def __init__(self, num_features, ghost_batch=32, eps=1e-5):
        super().__init__(num_features, eps=eps, track_running_stats=False)
        if int(ghost_batch) < 1:
            raise ValueError("ghost_batch must be a positive integer")
        self.ghost_batch = int(ghost_batch)

    def forward(self, x):
        ngroups = -(-x.shape[0] // self.ghost_batch)
        if ngroups <= 1:
            return super().forward(x)
        y = torch.empty_like(x)
        for g in range(ngroups):
            y[g::ngroups] = super().forward(x[g::ngroups])
        return y

    def extra_repr(self):
        return f"{super().extra_repr()}, ghost_batch={self.ghost_batch}"


def _make_layers(cfg, norm="batch", gn_groups=32, ghost_batch=32):
    """Same module sequence (and therefore the same Sequential indices) as part1/model.py:11-27.
    ``norm="group"``: nn.GroupNorm(gn_groups, v) where the BatchNorm sits (the same parameter
    names and shapes); ``norm="ghost"``: GhostBatchNorm2d(v, ghost_batch) there."""
    mods = []
    cin = 3
    for v in cfg:
        if v == 'M':
            mods.append(nn.MaxPool2d(kernel_size=2, stride=2))
            continue
        mods += [nn.Conv2d(cin, v, kernel_size=3, stride=1, padding=1, bias=True),
                 (nn.GroupNorm(gn_groups, v) if norm == "group"
                  else GhostBatchNorm2d(v, ghost_batch) if norm == "ghost"
                  else nn.BatchNorm2d(v, track_running_stats=False)),
                 nn.ReLU(inplace=True)]
        cin = v
    return nn.Sequential(*mods)


class _VGG(nn.Module):
    """VGG module for 3x32x32 input, ``num_classes`` classes (default 10)."""

    def __init__(self, name, num_classes=10, norm="batch", gn_groups=32, ghost_batch=32):
        super().__init__()
        if norm not in ("batch", "group", "ghost"):
            raise ValueError(f"unknown norm {norm}")
        self.name = name
        self.norm = norm
        self.ghost_batch = int(ghost_batch) if norm == "ghost" else None
        self.layers = _make_layers(_cfg[name], norm, gn_groups, ghost_batch)
        self.fc1 = nn.Linear(512, num_classes)
        self._plan = None

    # ------------------------------------------------------------ fused GPU plan
    def fused_plan(self):
        """Group the Sequential into ConvBNAct stages (built once per device)."""
        from ..ops.layers import ConvBNActSpec, ConvGNActSpec, ConvGhostBNActSpec
        dev = self.fc1.weight.device
        if self._plan is not None and self._plan[0] == dev:
            return self._plan[1]
        mods = list(self.layers)
        stages, i, first = [], 0, True
        while i < len(mods):
            conv = mods[i]
            if not isinstance(conv, nn.Conv2d):
                raise RuntimeError(f"unexpected module {conv} at layers.{i}")
            bn, relu = mods[i + 1], mods[i + 2]
            assert isinstance(bn, (nn.BatchNorm2d, nn.GroupNorm)) and isinstance(relu, nn.ReLU)
            pool = i + 3 < len(mods) and isinstance(mods[i + 3], nn.MaxPool2d)
            if isinstance(bn, nn.GroupNorm):
                # never chained: a GroupNorm block takes none of the BatchNorm fusions
                hw = 32 >> sum(isinstance(m, nn.MaxPool2d) for m in mods[:i])
                stages.append(ConvGNActSpec(conv, bn, relu=True, pool=pool, hw=(hw, hw),
                                            cin_pad=IN_CHANNELS_PADDED if first else None))
                first = False
                i += 4 if pool else 3
                continue
            if isinstance(bn, GhostBatchNorm2d):  # never chained either
                stages.append(ConvGhostBNActSpec(conv, bn, relu=True, pool=pool,
                                                 cin_pad=IN_CHANNELS_PADDED if first else None))
                first = False
                i += 4 if pool else 3
                continue
            spec = ConvBNActSpec(conv, bn, relu=True, pool=pool,
                                 cin_pad=IN_CHANNELS_PADDED if first else None)
            # this block's dgrad produces the gradient at the previous block's output: it
            # accumulates that block's BatchNorm-backward sums (ops.layers, BnBwdFuse)
            spec.prev = stages[-1] if stages else None
            if stages:
                stages[-1].next = spec
            stages.append(spec)
            first = False
            i += 4 if pool else 3
        self._plan = (dev, stages)
        return stages

    def packed_specs(self):
        return self.fused_plan() if self.fc1.weight.is_cuda else []

    def _features_fused(self, x):
        from ..ops.layers import conv_block, to_nhwc_input
        from ..ops.common import step_scratch
        plan = self.fused_plan()
        step_scratch(x.device).zero()  # BN statistics / backward sums of every layer: one fill
        h = to_nhwc_input(x, IN_CHANNELS_PADDED)
        for spec in plan:
            h = conv_block(h, spec)
        if h.shape[1] != 1 or h.shape[2] != 1:
            raise RuntimeError("VGG head expects 1x1 spatial features (32x32 input)")
        return h.view(h.shape[0], -1)  # NHWC with H=W=1: identical to the NCHW flatten

    def _head_cpu(self, y):
        """fc1 on the CPU. A ghost model applies it per ghost group, as its normalisation: ATen's
        GEMM rounds a row differently in a 16-row and an 8-row product, and per group the rows of
        a call are the same whatever the world size, so the logits are too. One group (and every
        other norm) is the plain call."""
        ngroups = -(-y.shape[0] // self.ghost_batch) if self.ghost_batch else 1
        if ngroups <= 1:
            return self.fc1(y)
        out = y.new_empty(y.shape[0], self.fc1.out_features)
        for g in range(ngroups):
            out[g::ngroups] = self.fc1(y[g::ngroups].contiguous())
        return out

    def forward(self, x):
        if not x.is_cuda:
            y = self.layers(x)
            y = y.view(y.size(0), -1)
            return self._head_cpu(y)
        from ..ops.layers import linear_small
        return linear_small(self._features_fused(x), self.fc1)

    @torch.no_grad()
    def forward_metrics(self, x, labels, loss_acc, correct_acc):
        """Evaluation in one classifier kernel (GPU): loss_acc (fp32 scalar) += mean CE of the
        batch, correct_acc (int32 scalar) += number of argmax hits (reference test_model,
        part1/main.py:96-111). No logits tensor, no host sync per batch."""
        from ..ops.common import native, ptr, stream_handle
        h = self._features_fused(x)
        B, F = h.shape
        labels = labels.to(torch.int64).contiguous()
        native().linear_ce_fwd(ptr(h), ptr(self.fc1.weight), ptr(self.fc1.bias), ptr(labels), B, F,
                               self.fc1.weight.shape[0], 0, 0, ptr(loss_acc), ptr(correct_acc),
                               stream_handle())

    def forward_loss_split(self, x, labels, split, acc=None, transient=False, soft=None):
        """``forward_loss`` cut after fused stage(s) ``split`` (GPU; an int or ascending list of
        stage indices): returns (loss, cuts) with cuts[k] = (h_k, leaf_k), h_k the output of the
        stages before split[k] and ``leaf_k = h_k.detach().requires_grad_()`` the input of the
        stages from split[k] on. ``loss.backward()`` produces the gradients of the stages from
        split[-1] (+ fc1) and ``h_k.backward(leaf_k.grad)`` for k = len-1 .. 0 those of each
        earlier segment — backward segments the DDP engine can put collectives between
        (engine/step.py SegmentedDDPStep). ``soft``: as in ``forward_loss``."""
        from ..ops.layers import conv_block, to_nhwc_input, linear_cross_entropy
        from ..ops.common import step_scratch
        plan = self.fused_plan()
        splits = [split] if isinstance(split, int) else list(split)
        if not splits or splits != sorted(set(splits)) or not 0 < splits[0] or splits[-1] >= len(plan):
            raise ValueError(f"split stages must be ascending in 1..{len(plan) - 1}")
        step_scratch(x.device).zero()
        h = to_nhwc_input(x, IN_CHANNELS_PADDED)
        cuts, prev = [], 0
        for sp in splits + [len(plan)]:
            for spec in plan[prev:sp]:
                h = conv_block(h, spec)
            if sp < len(plan):
                leaf = h.detach().requires_grad_(True)
                cuts.append((h, leaf))
                h = leaf
            prev = sp
        loss = linear_cross_entropy(h.view(h.shape[0], -1), self.fc1, labels, acc, transient,
                                    bn_prev=plan[-1] if self.norm == "batch" else None,
                                    soft=soft)
        return loss, cuts

    def n_stages(self):
        """Number of fused Conv->BN->ReLU(->pool) stages (cut points for forward_loss_split)."""
        return sum(1 for v in _cfg[self.name] if v != 'M')

    def first_param_of_stage(self, i):
        """Parameter that starts fused stage ``i`` in ``parameters()`` order (its conv weight)."""
        return self.fused_plan()[i].conv.weight

    def forward_loss(self, x, labels, acc=None, transient=False, soft=None):
        """``CrossEntropyLoss()(self(x), labels)`` with the classifier and the loss fused into one
        kernel on the GPU (engine/step.py uses it for the captured training step). ``acc`` (fp32
        scalar) additionally accumulates the loss across calls. The returned loss tensor is only
        valid until the next forward when ``transient`` (it then lives in the per-forward
        scratch and costs no fill launch). ``soft``: a SoftTarget (ops/common.py: label
        smoothing / mixup) in place of the one-hot target, in the same kernel."""
        if not x.is_cuda:
            if soft is not None:
                loss = soft.torch_loss(self.forward(x), labels)
            else:
                loss = nn.functional.cross_entropy(self.forward(x), labels)
            if acc is not None:
                acc.add_(loss.detach())
            return loss
        from ..ops.layers import HEAD_NARROW_MAX, linear_cross_entropy
        if self.norm != "batch":  # no BatchNorm to fold into the head: it reads stored features
            return linear_cross_entropy(self._features_fused(x), self.fc1, labels, acc, transient,
                                        bn_prev=None, soft=soft)
        last = self.fused_plan()[-1]
        # its BN + ReLU + pool may run inside the narrow head's kernel; the wide head (more than 16
        # classes) reads stored features, so the block then runs its own pass
        last.defer_to_head = self.fc1.weight.shape[0] <= HEAD_NARROW_MAX
        try:
            h = self._features_fused(x)
        finally:
            last.defer_to_head = False
        return linear_cross_entropy(h, self.fc1, labels, acc, transient, bn_prev=last, soft=soft)


def VGG11(num_classes=10, norm="batch", gn_groups=32, ghost_batch=32):
    return _VGG('VGG11', num_classes, norm, gn_groups, ghost_batch)


def VGG13(num_classes=10, norm="batch", gn_groups=32, ghost_batch=32):
    return _VGG('VGG13', num_classes, norm, gn_groups, ghost_batch)


def VGG16(num_classes=10, norm="batch", gn_groups=32, ghost_batch=32):
    return _VGG('VGG16', num_classes, norm, gn_groups, ghost_batch)


def VGG19(num_classes=10, norm="batch", gn_groups=32, ghost_batch=32):
    return _VGG('VGG19', num_classes, norm, gn_groups, ghost_batch)
