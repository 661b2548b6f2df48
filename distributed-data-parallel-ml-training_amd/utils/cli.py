"""Command-line contract of the reference mains.

Reference parity: ``parse_arguments`` (part2/part2a/main.py:20-32, part3/main.py:21-33) with
exactly four flags — ``--master-ip`` (str, default 10.10.1.1), ``--master-port`` (str, default
'4000'), ``--num-nodes`` (int, dest ``size``), ``--rank`` (int, default from the hostname
``nodeK`` via ``get_rank``, part2/part2a/main.py:35-39) — returning ``(ip, port, rank, size)``.

Fixed defects: the rank default is resolved LAZILY and non-fatally
(RANK env -> digit at hostname[4] -> 0) instead of crashing while the parser is built, and a
missing ``--num-nodes`` falls back to WORLD_SIZE (or 1). Opt-in flags add device / data / model /
perf controls without changing any reference default.
"""
import argparse
import os


def get_rank():
    """RANK env (torchrun), else the digit of a CloudLab-style hostname ``nodeK``, else 0."""
    if "RANK" in os.environ:
        return int(os.environ["RANK"])
    name = os.uname().nodename
    if len(name) > 4 and name[4].isdigit():
        return int(name[4])
    return 0


def build_parser(description=None, distributed=True):
    p = argparse.ArgumentParser(description=description)
    if distributed:
        p.add_argument('--master-ip', dest='master_ip', default=os.environ.get("MASTER_ADDR", "10.10.1.1"),
                       type=str, help='Speficy master ip. Default is 10.10.1.1')
        p.add_argument('--master-port', dest='master_port', default=os.environ.get("MASTER_PORT", '4000'),
                       type=str, help='Specify master port. Default is 4000.')
        p.add_argument('--num-nodes', dest='size', type=int, default=None,
                       help='Specify the number of nodes to distribute training over.')
        p.add_argument('--rank', dest='rank', default=None, type=int,
                       help='Specify the rank for this machine. The default takes the number from '
                            'the computer name.')
    g = p.add_argument_group("ddp_amd extensions (opt-in; reference defaults unchanged)")
    g.add_argument('--device', default='auto', help='auto | cpu | cuda')
    g.add_argument('--model', default='vgg11', help='vgg11 | vgg13 | vgg16 | vgg19 | resnet50')
    g.add_argument('--epochs', type=int, default=1)
    g.add_argument('--global-batch', type=int, default=256, help='split int(B/world) per rank')
    g.add_argument('--train-size', type=int, default=None, help='synthetic train-set size')
    g.add_argument('--test-size', type=int, default=None, help='synthetic test-set size')
    g.add_argument('--max-batches', type=int, default=None, help='stop the epoch early')
    g.add_argument('--bucket-mb', type=_mb, default=25.0,
                   help="DDP bucket cap (MiB; default 25 = the reference's torch DDP default); "
                        "'auto' = sized from the all-reduce bandwidth table "
                        "(parallel/comm_tuning.json)")
    g.add_argument('--first-bucket-mb', type=_mb, default=1.0)
    g.add_argument('--threads', type=int, default=4, help='torch CPU threads (reference: 4)')
    g.add_argument('--save', default=None, help='write a reference-layout checkpoint here')
    g.add_argument('--resume', default=None, help='load a checkpoint before training')
    g.add_argument('--metrics', default=None, help='JSON-lines metrics sink')
    g.add_argument('--no-test', action='store_true', help='skip the evaluation pass')
    g.add_argument('--watchdog-s', type=float, default=300.0,
                   help='distributed runs: abort + exit non-zero after this many seconds '
                        'without a finished iteration (0 = off)')
    g.add_argument('--graph', action='store_true',
                   help='GPU: run each iteration as one replay of the captured training step')
    g.add_argument('--lr', type=float, default=0.1, help='base learning rate (reference: 0.1)')
    g.add_argument('--lr-schedule', default=None, choices=['constant', 'cosine', 'linear', 'step'],
                   help='per-step learning-rate schedule over epochs x steps-per-epoch steps '
                        '(works inside the captured step of --graph); default: none, constant --lr')
    g.add_argument('--warmup-steps', type=int, default=0,
                   help='linear warm-up from 0 to the base rate over this many steps')
    g.add_argument('--lr-milestones', type=_int_list, default=[],
                   help="--lr-schedule step: comma-separated global steps at which the rate is "
                        "multiplied by --lr-gamma")
    g.add_argument('--lr-gamma', type=float, default=0.1)
    g.add_argument('--min-lr', type=float, default=0.0, help='end value of cosine / linear')
    g.add_argument('--lr-ref-batch', type=int, default=None,
                   help='linear scaling rule: lr *= global batch / this batch')
    g.add_argument('--optimizer', default='sgd', choices=['sgd', 'lars', 'adamw', 'lamb'],
                   help='sgd (reference) | lars: every weight tensor\'s update scaled by its trust '
                        'ratio eta |w| / (|g| + wd |w| + eps), for the learning rates that the '
                        'linear scaling rule gives a large global batch (works inside --graph) | '
                        'adamw: Adam with decoupled weight decay (torch.optim.AdamW) inside the '
                        'update launch (works inside --graph; pass an Adam-sized --lr, 0.001) | '
                        'lamb: the AdamW update with every weight tensor\'s step scaled by its '
                        'trust ratio |w| / |update|, for Adam at a large global batch (one more '
                        'launch per update; works inside --graph)')
    g.add_argument('--adam-beta1', type=_adam_beta, default=0.9)
    g.add_argument('--adam-beta2', type=_adam_beta, default=0.999)
    g.add_argument('--adam-eps', type=_non_negative('--adam-eps'), default=1e-8)
    g.add_argument('--weight-decay', type=_non_negative('--weight-decay'), default=None,
                   help="weight decay; default: the optimizer's own, 1e-4 for sgd and lars "
                        "(reference), 1e-2 for adamw and lamb")
    g.add_argument('--lars-eta', type=float, default=0.001, help='LARS trust coefficient')
    g.add_argument('--lars-eps', type=float, default=1e-8)
    g.add_argument('--clip-grad-norm', type=float, default=None,
                   help='clip the 2-norm of the whole gradient to this value inside the update '
                        'launch (torch.nn.utils.clip_grad_norm_; works inside --graph); default off')
    g.add_argument('--skip-nonfinite-grads', action='store_true',
                   help='a step whose gradient norm is Inf / NaN changes no parameter and is '
                        'counted instead (works inside --graph); default off')
    g.add_argument('--accum-steps', type=_accum_steps, default=1,
                   help='gradient accumulation: one optimizer step consumes this many consecutive '
                        'batches of --global-batch samples (effective batch = global batch x K; one '
                        'gradient sync and one update per K backward passes; works inside --graph)')
    g.add_argument('--label-smoothing', type=_label_smoothing, default=0.0,
                   help='training loss against (1 - E) * target + E / classes, 0 <= E < 1 '
                        '(torch label_smoothing; inside the fused loss kernels, works inside '
                        '--graph; evaluation stays the plain loss); default 0')
    g.add_argument('--mixup-alpha', type=_mixup_alpha, default=0.0,
                   help='mixup: every training batch is blended with itself reversed by lam ~ '
                        'Beta(A, A), one draw per batch from a per-epoch table, inside the batch '
                        'kernel, and the loss is lam * CE(y) + (1 - lam) * CE(y reversed) (works '
                        'inside --graph); default 0 = off')
    g.add_argument('--ema-decay', type=_ema_decay, default=0.0,
                   help='exponential moving average of the weights with this decay, 0 <= D < 1, '
                        'advanced once per optimizer step inside the update launch (works inside '
                        '--graph); a second evaluation pass runs on the averaged weights and '
                        '--save stores them as ema_state_dict; default 0 = off')
    g.add_argument('--no-decay-1d', action='store_true',
                   help='no weight decay on biases and BatchNorm gamma / beta (every parameter '
                        'with dim() <= 1), the usual second param group of SGD, LARS, AdamW and '
                        'LAMB recipes, decided per work item inside the update launch (works '
                        'inside --graph); default off')
    return p


def _adam_beta(v):
    b = float(v)
    if not 0.0 <= b < 1.0:
        raise argparse.ArgumentTypeError("an Adam beta must be in [0, 1)")
    return b


def _non_negative(flag):
    def parse(v):
        x = float(v)
        if not (x >= 0.0 and x != float("inf")):
            raise argparse.ArgumentTypeError(f"{flag} must be a finite number >= 0")
        return x
    return parse


def _ema_decay(v):
    d = float(v)
    if not 0.0 <= d < 1.0:
        raise argparse.ArgumentTypeError("--ema-decay must be in [0, 1)")
    return d


def _label_smoothing(v):
    e = float(v)
    if not 0.0 <= e < 1.0:
        raise argparse.ArgumentTypeError("--label-smoothing must be in [0, 1)")
    return e


def _mixup_alpha(v):
    a = float(v)
    if not (a >= 0.0 and a != float("inf")):
        raise argparse.ArgumentTypeError("--mixup-alpha must be a finite number >= 0")
    return a


def _accum_steps(v):
    k = int(v)
    if k < 1:
        raise argparse.ArgumentTypeError("--accum-steps must be >= 1")
    return k


def optimizer_from_args(args, params, lr):
    """The run's optimizer: the reference's SGD(lr, 0.9, 1e-4), or LARS over the same
    hyper-parameters with --optimizer lars (biases and BatchNorm vectors are not adapted), or
    AdamW(lr, (--adam-beta1, --adam-beta2), --adam-eps, 1e-2) with --optimizer adamw, or LAMB over
    AdamW's hyper-parameters with --optimizer lamb (biases and BatchNorm vectors are not adapted);
    --weight-decay replaces the optimizer's default decay; --clip-grad-norm /
    --skip-nonfinite-grads switch the gradient guard of any of them on; --no-decay-1d takes the
    decay off biases and BatchNorm vectors in any of them."""
    from ..optim import FusedSGD, LAMB, LARS, AdamW
    guard = {}
    if getattr(args, "clip_grad_norm", None) is not None or \
            getattr(args, "skip_nonfinite_grads", False):
        guard = {"max_grad_norm": getattr(args, "clip_grad_norm", None),
                 "skip_nonfinite": bool(getattr(args, "skip_nonfinite_grads", False))}
    if getattr(args, "no_decay_1d", False):
        guard = dict(guard, no_decay="1d")
    wd = getattr(args, "weight_decay", None)
    if getattr(args, "optimizer", "sgd") in ("adamw", "lamb"):
        cls = LAMB if args.optimizer == "lamb" else AdamW
        return cls(params, lr=lr, betas=(getattr(args, "adam_beta1", 0.9),
                                         getattr(args, "adam_beta2", 0.999)),
                   eps=getattr(args, "adam_eps", 1e-8),
                   weight_decay=0.01 if wd is None else wd, **guard)
    wd = 0.0001 if wd is None else wd
    if getattr(args, "optimizer", "sgd") == "lars":
        return LARS(params, lr=lr, momentum=0.9, weight_decay=wd,
                    trust_coefficient=args.lars_eta, eps=args.lars_eps, **guard)
    return FusedSGD(params, lr=lr, momentum=0.9, weight_decay=wd, **guard)


def lr_schedule_from_args(args, steps_per_epoch):
    """(base lr, LRSchedule | None) of a run: the linear scaling rule applied to --lr, and a
    schedule over epochs x steps_per_epoch steps (the partial last batch of an epoch is a step)
    only when --lr-schedule or --warmup-steps asks for one. ``steps_per_epoch`` counts loader
    batches; with --accum-steps K the effective batch is global batch x K and an epoch has
    ceil(steps_per_epoch / K) optimizer steps (the leftover micro-batches form one)."""
    lr = float(args.lr)
    accum = int(getattr(args, "accum_steps", 1) or 1)
    if args.lr_ref_batch:
        lr *= args.global_batch * accum / float(args.lr_ref_batch)
    if args.lr_schedule is None and not args.warmup_steps:
        return lr, None
    from ..optim.schedule import LRSchedule
    steps_per_epoch = -(-int(steps_per_epoch) // accum)
    total = max(1, int(args.epochs) * int(steps_per_epoch))
    return lr, LRSchedule(lr, total, warmup_steps=min(int(args.warmup_steps), total),
                          decay=args.lr_schedule or "constant", milestones=args.lr_milestones,
                          gamma=args.lr_gamma, min_lr=args.min_lr)


def _int_list(v):
    return [int(x) for x in str(v).split(",") if x.strip()]


def finalize_args(args):
    if hasattr(args, "rank"):
        if args.rank is None:
            args.rank = get_rank()
        if args.size is None:
            args.size = int(os.environ.get("WORLD_SIZE", "1"))
    return args


def parse_arguments(argv=None):
    """Reference-shaped: returns (master_ip, master_port, rank, size)."""
    args = finalize_args(build_parser().parse_args(argv))
    return args.master_ip, args.master_port, args.rank, args.size


def _mb(v):
    return v if v == "auto" else float(v)


def parse_all(argv=None, distributed=True, description=None):
    return finalize_args(build_parser(description, distributed).parse_args(argv))
