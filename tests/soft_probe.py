"""Label smoothing + mixup in the deterministic-statistics build (run as a subprocess of
tests/test_gpu_soft_targets_model.py with DDP_AMD_DETERMINISTIC=1; prints one JSON line).
VGG-11, batch 8, 64 samples, label_smoothing 0.1, mixup alpha 0.4, 3 steps; every comparison
is torch.equal (tests/accum_probe.py Rig / same).

    python tests/soft_probe.py paths   # eager == captured TrainStep, K = 1 and K = 2; the lam
                                       #   each micro-batch published == the table's entries
"""
import json
import sys

from accum_probe import B, Rig, _base, _setup, same

E, ALPHA, STEPS = 0.1, 0.4, 3


def _rig(base):
    from ddp_amd.data import DeviceLoader, SyntheticCIFAR10
    rig = Rig(base)
    rig.ld = DeviceLoader(SyntheticCIFAR10(True, n=64), B, "cuda", mixup_alpha=ALPHA)
    return rig


def paths_case():
    torch = _setup()
    from ddp_amd.engine import CrossEntropyLoss, TrainStep
    base = _base()
    res = {}
    for K in (1, 2):
        rig = _rig(base)
        plain = Rig(base)
        table = [float(v) for v in rig.ld.lam_table]
        res[f"K{K}/table"] = len(table) == 8 and len(set(table)) == 8
        st = TrainStep(rig.model, rig.opt, CrossEntropyLoss(label_smoothing=E), rig.ld,
                       accum_steps=K)
        lams = []

        def recorded(fn):
            def run():
                fn()
                lams.append(st.lams())
            return run
        eager = rig.run(recorded(st._body), steps=STEPS)
        want = [table[i * K:(i + 1) * K] for i in range(STEPS)]
        res[f"K{K}/eager_lams"] = lams == want
        res[f"K{K}/moved"] = not torch.equal(eager["p"], rig.snap[0])
        res[f"K{K}/cursor"] = eager["cursor"] == STEPS * K
        # the flags change the step: the same steps with the plain loss and batches differ
        pst = TrainStep(plain.model, plain.opt, CrossEntropyLoss(), plain.ld, accum_steps=K)
        res[f"K{K}/differs_from_plain"] = not torch.equal(
            plain.run(pst._body, steps=STEPS)["p"], eager["p"])
        st.warmup(1)
        st.capture()
        del lams[:]
        res[f"K{K}/captured_equals_eager"] = same(eager, rig.run(recorded(st.step), steps=STEPS))
        res[f"K{K}/captured_lams"] = lams == want
        # an eager step on an explicit mixed batch reports its own lam, the replay after it
        # the captured step's again (cursor = STEPS * K)
        st.tail_step([(*rig.ld.batch(0, B), rig.ld.soft_targets())])
        res[f"K{K}/tail_lam"] = st.lams() == table[:1]
        st.step()
        res[f"K{K}/replay_after_tail_lams"] = st.lams() == table[STEPS * K:STEPS * K + K]
    return res


def main():
    print(json.dumps({"paths": paths_case}[sys.argv[1]]()))


if __name__ == "__main__":
    main()
