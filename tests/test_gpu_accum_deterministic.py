"""Gradient accumulation, bit for bit, in the deterministic-statistics build (tests/accum_probe.py,
one subprocess per case: the extension is loaded once per process). There a training step is a
deterministic function of its inputs, so the accumulated gradient must be the in-order fp32 sum of
the micro-batches' gradients, and every way of running the accumulated step -- eager, captured,
made by hand from accumulate-only micro-steps and the plain update launch, pipelined with the
all-reduce or the sharded plan, clipped, LARS -- must leave the same masters, momentum, bf16
operand copies and cursor."""
import json
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _probe(case):
    env = dict(os.environ, DDP_AMD_DETERMINISTIC="1")
    env.pop("DDP_AMD_SGD_IN_BWD", None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "accum_probe.py"), case],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(case, res)
    return res


def _all_true(res):
    bad = {k: v for k, v in res.items() if v is not True}
    assert not bad, bad


def test_accumulated_gradient_is_the_in_order_sum(native_ext):
    """Three accumulate-only micro-steps against the three gradients computed alone from a zeroed
    arena with the same weights, added in order in fp32: every producer adds exactly its own
    fixed-order total onto what is there (an overwriting or re-ordered one shows up here)."""
    res = _probe("sum")
    where = (res.pop("differing"), res.pop("differing_params"))
    bad = {k: v for k, v in res.items() if v is not True}
    assert not bad, (bad, where)


def test_accumulated_step_paths_agree(native_ext):
    """K = 2 and K = 3 (a scale that is no power of two), two optimizer steps from one state."""
    res = _probe("paths")
    for K in (2, 3):
        assert res.pop(f"K{K}/opt_in_bwd") is False  # never in the backward with K > 1
    _all_true(res)


def test_k1_is_the_plain_step(native_ext):
    _all_true(_probe("k1"))


def test_pipelined_accumulated_step_equals_train_step(native_ext):
    res = _probe("ddp")
    diag = res.pop("diag_k1_cut_equals_uncut")
    bad = {k: v for k, v in res.items() if v is not True}
    assert not bad, (bad, {"k1_cut_equals_uncut": diag})


def test_accumulated_step_with_the_gradient_guard_and_lars(native_ext):
    """Eager == captured with max_grad_norm and with LARS, and the guard's norm is the norm of
    the accumulated gradient x 1/2. Bound: tests/test_gpu_grad_clip.py's derivation (serial
    chains of rounded non-negative additions: 33 per thread + 6 + 3 in the sum-of-squares launch;
    in the update launch a lane adds ceil(chunks / 64) partials, then 6 wave levels; the square
    root halves the relative error and rounds once), with this arena's chunk count; the
    reference is the fp64 norm of the fp32 gradient times the exact factor 1/2."""
    res = _probe("guard")
    assert res.pop("guard/opt_in_bwd") is False and res.pop("lars/opt_in_bwd") is False
    got, want = res.pop("guard/norm"), res.pop("guard/norm_want")
    again = res.pop("guard/norm_replayed")
    chain = 33 + 6 + 3 + math.ceil(res.pop("guard/n_chunks") / 64) + 6
    rtol = (chain / 2 + 1) * 2.0 ** -24
    print(f"norm {got!r} want {want!r} rel err {abs(got - want) / want:.3e} bound {rtol:.3e}")
    assert want > 0 and abs(got - want) <= rtol * want
    assert again > 0 and again == again
    _all_true(res)


def test_captured_k1_loop_with_a_partial_last_batch(native_ext):
    """train_model_graph with K = 1 over 60 samples at batch 8, the default TrainStep (SGD in
    the backward) and the cosine schedule: 7 replays and one eager step on the partial batch of
    4 leave, bit for bit, what seven ``_body()`` and one ``tail_step(*ld.batch(56, 4))`` leave;
    8 metrics records without ``accum``, graph_replays 7, cursor 7, the schedule step 8 on the
    device and in its host mirror, the records' ``lr`` the schedule's entries 0..7, and a
    clear gradient arena."""
    res = _probe("loop1")
    assert res.pop("opt_in_bwd") is True
    _all_true(res)


def test_leftover_step_and_eager_loop_equal_the_hand_made_step(native_ext):
    """TrainStep.tail_step on a list of micro-batches (two full ones and a partial one: m = 3,
    a scale that is no power of two), the same list through SegmentedDDPStep.tail_step, and the
    eager loop train_model(accum_steps=2) on the GPU, each bit for bit against plain backward
    passes followed by one update at float32(1 / m)."""
    _all_true(_probe("tail"))
