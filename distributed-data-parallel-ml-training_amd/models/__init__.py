"""Model zoo: VGG-11/13/16/19 (reference family) and ResNet-50 (driver's large-gradient config)."""
from .vgg import VGG11, VGG13, VGG16, VGG19, _VGG  # noqa: F401


def build(name, num_classes=None):
    """``num_classes``: the head's output count; None = the model's default."""
    name = name.lower()
    kw = {} if num_classes is None else {"num_classes": int(num_classes)}
    table = {"vgg11": VGG11, "vgg13": VGG13, "vgg16": VGG16, "vgg19": VGG19}
    if name in table:
        return table[name](**kw)
    if name in ("resnet50", "resnet-50"):
        from .resnet import resnet50
        return resnet50(**kw)
    raise ValueError(f"unknown model {name}")
