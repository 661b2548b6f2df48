"""--norm ghost on the CPU: the model tree and checkpoint layout, GhostBatchNorm2d against
per-group F.batch_norm, the one-group case, world-size invariance, the command line. No GPU."""
import pytest
import torch
import torch.nn.functional as F


def _models(ghost):
    from ddp_amd.models import build
    torch.manual_seed(3)
    bn, gh = build("vgg11"), build("vgg11", norm="ghost", ghost_batch=ghost)
    gh.load_state_dict(bn.state_dict())
    return bn, gh


def test_ghost_checkpoint_layout_and_one_group_is_batch_norm():
    bn, gh = _models(16)
    sa, sb = bn.state_dict(), gh.state_dict()
    assert list(sa) == list(sb)
    assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]
    x = torch.randn(16, 3, 32, 32)
    with torch.no_grad():
        assert torch.equal(gh(x), bn(x))           # ghost_batch >= N: one group
        assert not torch.equal(gh(torch.cat([x, x[:4]])), bn(torch.cat([x, x[:4]])))


@pytest.mark.parametrize("N,G", [(8, 4), (7, 3), (5, 8)])
def test_ghost_batch_norm_is_per_group_batch_norm(N, G):
    from ddp_amd.models import GhostBatchNorm2d
    torch.manual_seed(N)
    m = GhostBatchNorm2d(6, G)
    m.weight.data.uniform_(0.5, 1.5)
    m.bias.data.normal_()
    assert not m.track_running_stats and m.running_mean is None
    x = torch.randn(N, 6, 3, 5)
    ng = -(-N // G)
    y = m(x)
    for g in range(ng):
        want = F.batch_norm(x[g::ng], None, None, m.weight, m.bias, True, 0.0, m.eps)
        assert torch.equal(y[g::ng], want), g
    assert torch.equal(m.eval()(x), y)  # no running statistics: eval takes the same path


def _whole_and_sharded(fn, x, width):
    """fn(whole batch) and fn(rank r's share x[r::2], the sharded sampler's deal) put back."""
    with torch.no_grad():
        whole, parts = fn(x), torch.empty(x.shape[0], width)
        for r in range(2):
            parts[r::2] = fn(x[r::2])
    return whole, parts


def test_ghost_features_do_not_depend_on_the_world_size():
    """Batch 16, ghost 4: everything up to the head is the same bits for one rank of 16 and two
    ranks of 8; BatchNorm's local-batch statistics break exactly that."""
    bn, gh = _models(4)
    x = torch.randn(16, 3, 32, 32)
    whole, parts = _whole_and_sharded(lambda t: gh.layers(t).flatten(1), x, 512)
    assert torch.equal(whole, parts)
    whole, parts = _whole_and_sharded(lambda t: bn.layers(t).flatten(1), x, 512)
    assert not torch.allclose(whole, parts)


def test_ghost_logits_do_not_depend_on_the_world_size():
    """The same comparison on the logits, to torch.allclose's default tolerances (rtol 1e-5, atol
    1e-8); BatchNorm fails it. nn.Linear's 16-row and 8-row GEMMs round a row differently (6.0e-7
    here, 2.2e-5 of a logit of 0.027), which is why the ghost model's CPU head runs per ghost
    group (models/vgg.py ``_head_cpu``)."""
    bn, gh = _models(4)
    x = torch.randn(16, 3, 32, 32)
    assert not torch.allclose(*_whole_and_sharded(bn, x, 10))
    assert torch.allclose(*_whole_and_sharded(gh, x, 10))


def test_cli_and_build_refusals():
    from ddp_amd.models import GhostBatchNorm2d, build
    from ddp_amd.utils.cli import parse_all
    args = parse_all(["--norm", "ghost", "--ghost-batch", "8"], distributed=False)
    assert (args.norm, args.ghost_batch) == ("ghost", 8)
    assert parse_all([], distributed=False).ghost_batch == 32
    with pytest.raises(SystemExit):
        parse_all(["--ghost-batch", "0"], distributed=False)
    m = build(args.model, norm=args.norm, ghost_batch=args.ghost_batch)
    assert isinstance(m.layers[1], GhostBatchNorm2d) and m.layers[1].ghost_batch == 8
    with pytest.raises(ValueError, match="--norm ghost is served for vgg11/13/16/19"):
        build("resnet50", norm="ghost")
