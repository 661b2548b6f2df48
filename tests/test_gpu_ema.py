"""Weight EMA (--ema-decay, optim/sgd.py set_ema) inside the training steps: tests/ema_probe.py,
one fresh child process per mode (the extension is loaded once per process). VGG-11, batch 32,
decay 0.9, 4 optimizer steps.

* deterministic build: a step is a deterministic function of its inputs there, so the eager loop
  and the captured TrainStep must end with torch.equal masters and EMA -- plain, with
  --accum-steps 2 (the EMA advances once per optimizer step), and with LARS plus clipping;
* release build: the EMA is a deterministic function of the masters, so the captured step's EMA
  must equal the fp32 lerp recurrence over the masters snapshotted after each replay, bit for
  bit;
* dispatches: the EMA adds no launch of its own. With it off a captured b32 step has the 41
  dispatches it had before; with it on it has those of the step without SGD in the backward
  (DDP_AMD_SGD_IN_BWD=0), which is what giving up the updates in the WGRAD finishes costs.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _probe(case, det=False):
    env = dict(os.environ)
    env.pop("DDP_AMD_SGD_IN_BWD", None)
    env.pop("DDP_AMD_DETERMINISTIC", None)
    if det:
        env["DDP_AMD_DETERMINISTIC"] = "1"
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "ema_probe.py"), case],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(case, res)
    return res, r.stderr


def test_eager_equals_captured_deterministic(native_ext):
    res, _ = _probe("det", det=True)
    assert len(res) == 3 * 7 + 1
    bad = {k: v for k, v in res.items() if v is not True}
    assert not bad, bad


def test_captured_ema_is_the_recurrence_over_the_masters(native_ext):
    res, _ = _probe("release")
    differing = res.pop("differing")
    bad = {k: v for k, v in res.items() if v is not True}
    assert not bad, (bad, differing)


def test_ema_adds_no_dispatch(native_ext):
    res, names = _probe("count")
    assert res["off/opt_in_bwd"] is True and res["on/opt_in_bwd"] is False
    assert res["off_no_in_bwd/opt_in_bwd"] is False
    assert res["off"] == 41, names[-4000:]
    assert res["on"] == res["off_no_in_bwd"], names[-4000:]
    assert res["on/update_launches"] == res["off_no_in_bwd/update_launches"] == 1
