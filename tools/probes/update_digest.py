"""State digests of the update launch in the deterministic-statistics build, to compare two
source trees bit for bit (profiles/update_kernels_refactor.md).

    cd <root of a tree> && DDP_AMD_DETERMINISTIC=1 python <this file>

It imports tests/accum_probe.py of the tree it is run in (the current directory) and prints one
JSON line: per configuration the SHA-256 over masters, momentum, every bf16 operand copy, the
cursor and the schedule step after two captured steps (accum_probe's "state" digest, without the
loss meter). Configurations: plain SGD and LARS, gradient guard off and on, K = 1 and 2 with
every update in the step's own launch, plus the default K = 1 step with SGD in the backward."""
import contextlib
import io
import json
import os
import sys

ROOT = os.getcwd()
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import accum_probe as ap  # noqa: E402


def main():
    ap._setup()
    from ddp_amd.optim import LARS
    base = ap._base()
    res = {}
    guard = dict(max_grad_norm=1e-3, skip_nonfinite=True)

    def one(name, K, **kw):
        rig = ap.Rig(base, **kw)
        ap._sched(rig.opt)
        st = ap._step(rig, K)
        st.warmup(2)
        st.capture()
        err = io.StringIO()
        with contextlib.redirect_stderr(err):
            ap._digest(rig, st.step, st)
        words = err.getvalue().split()
        res[name] = words[words.index("state") + 1]
        extra = {}
        if rig.opt.guarded:
            extra = dict(norm=float(rig.opt.grad_norm()), c=float(rig.opt.clip_coef()),
                         skipped=int(rig.opt.skipped_steps()))
        print(name, res[name], "in_bwd", st.opt_in_bwd, extra, file=sys.stderr, flush=True)

    one("sgd/K1/in_bwd", 1)
    os.environ["DDP_AMD_SGD_IN_BWD"] = "0"
    for K in (1, 2):
        one(f"sgd/K{K}", K)
        one(f"sgd+guard/K{K}", K, **guard)
        one(f"lars/K{K}", K, opt_cls=LARS, trust_coefficient=0.02)
        one(f"lars+guard/K{K}", K, opt_cls=LARS, trust_coefficient=0.02, **guard)
    print(json.dumps(res))


main()
