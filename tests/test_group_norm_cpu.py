"""--norm group on the CPU: the model tree, the checkpoint layout, batch-split invariance, the
command line and the optimizers' vector rules. No GPU."""
import pytest
import torch
import torch.nn as nn


def _models():
    from ddp_amd.models import build
    torch.manual_seed(3)
    return build("vgg11"), build("vgg11", norm="group")


def test_group_model_tree_and_checkpoint_layout():
    bn, gn = _models()
    for i, (a, b) in enumerate(zip(bn.layers, gn.layers)):
        if isinstance(a, nn.BatchNorm2d):
            assert isinstance(b, nn.GroupNorm), i
            assert (b.num_groups, b.num_channels) == (32, a.num_features), i
        else:
            assert type(a) is type(b), i
    sa, sb = bn.state_dict(), gn.state_dict()
    assert list(sa) == list(sb)
    assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]
    gn.load_state_dict(sa)  # key for key (it then means something else)
    from ddp_amd.models import build
    assert build("vgg16", norm="group", gn_groups=8).layers[1].num_groups == 8


def test_group_forward_is_batch_split_invariant():
    """logits(16 images) == cat(logits(first 8), logits(last 8)) to fp32 rounding with
    GroupNorm; BatchNorm's local-batch statistics break exactly that."""
    bn, gn = _models()
    x = torch.randn(16, 3, 32, 32)
    with torch.no_grad():
        whole, halves = gn(x), torch.cat([gn(x[:8]), gn(x[8:])])
        bwhole, bhalves = bn(x), torch.cat([bn(x[:8]), bn(x[8:])])
    scale = float(whole.abs().max())
    assert float((whole - halves).abs().max()) <= 1e-5 * scale
    assert float((bwhole - bhalves).abs().max()) > 1e-3 * float(bwhole.abs().max())


def test_cli_and_build_refusals():
    from ddp_amd.models import build
    from ddp_amd.utils.cli import parse_all
    args = parse_all(["--norm", "group", "--gn-groups", "8"], distributed=False)
    assert (args.norm, args.gn_groups) == ("group", 8)
    d = parse_all([], distributed=False)
    assert (d.norm, d.gn_groups) == ("batch", 32)
    with pytest.raises(ValueError, match="--norm group is served for vgg11/13/16/19"):
        build("resnet50", norm="group")


def test_no_decay_1d_covers_group_norm_vectors():
    from ddp_amd.optim import FusedSGD
    _, gn = _models()
    opt = FusedSGD(gn.parameters(), lr=0.1, weight_decay=1e-4, no_decay="1d")
    mask = opt.no_decay_mask
    for (n, p), masked in zip(gn.named_parameters(), mask):
        assert masked == (p.dim() <= 1), n
    idx = [i for i, (n, _) in enumerate(gn.named_parameters()) if n.startswith("layers.1.")]
    assert len(idx) == 2 and all(mask[i] for i in idx)  # GroupNorm's gamma and beta
