"""Model zoo: VGG-11/13/16/19 (reference family) ResNet-50 (driver's large-gradient config),
ResNeXt-50 32x4d (the same module tree with a grouped conv2), their Squeeze-and-Excitation
variants, MobileNet v1 (depthwise-separable
blocks) and RepVGG-A0 / A1 (three-branch BatchNorm blocks)."""
from .vgg import VGG11, VGG13, VGG16, VGG19, _VGG, GhostBatchNorm2d  # noqa: F401


def build(name, num_classes=None, norm="batch", gn_groups=32, ghost_batch=32):
    """``num_classes``: the head's output count; None = the model's default. ``norm``: "batch"
    (BatchNorm over the local batch), "group" (GroupNorm with ``gn_groups`` groups: per-image
    statistics; the VGG family) or "ghost" (BatchNorm over interleaved groups of ``ghost_batch``
    images: the same function for every per-GPU batch share; the VGG family)."""
    name = name.lower()
    kw = {} if num_classes is None else {"num_classes": int(num_classes)}
    table = {"vgg11": VGG11, "vgg13": VGG13, "vgg16": VGG16, "vgg19": VGG19}
    if norm not in ("batch", "group", "ghost"):
        raise ValueError(f"unknown norm {norm}")
    if norm == "ghost":
        if name not in table:
            raise ValueError("--norm ghost is served for vgg11/13/16/19")
        return table[name](norm="ghost", ghost_batch=int(ghost_batch), **kw)
    if norm == "group":
        if name not in table:
            raise ValueError("--norm group is served for vgg11/13/16/19")
        return table[name](norm="group", gn_groups=int(gn_groups), **kw)
    if name in table:
        return table[name](**kw)
    if name in ("resnet50", "resnet-50"):
        from .resnet import resnet50
        return resnet50(**kw)
    # "resnet50_32x4d" is an alias: bench.py and engine/step.py default_cuts recognise the ResNet
    # family by startswith("resnet"), so that spelling runs ResNeXt-50 through both unchanged
    if name in ("resnext50_32x4d", "resnet50_32x4d"):
        from .resnet import resnext50_32x4d
        return resnext50_32x4d(**kw)
    # the Squeeze-and-Excitation variants (csrc/kernels/se.hip); the "resnet..." spellings are
    # aliases for the same reason
    if name in ("se_resnet50", "resnet50_se"):
        from .resnet import se_resnet50
        return se_resnet50(**kw)
    if name in ("se_resnext50_32x4d", "resnet50_32x4d_se"):
        from .resnet import se_resnext50_32x4d
        return se_resnext50_32x4d(**kw)
    if name in ("mobilenet_v1", "mobilenet"):
        from .mobilenet import mobilenet_v1
        return mobilenet_v1(**kw)
    # RepVGG in training form (three-branch blocks, csrc/kernels/rep_bn.hip)
    if name in ("repvgg_a0", "repvgg_a1"):
        from .repvgg import repvgg
        return repvgg(name, **kw)
    raise ValueError(f"unknown model {name}")
