"""Gradient accumulation over two Gloo ranks (CPU): the eager loop syncs gradients once per
optimizer step -- DDP launches each bucket once, 2A / 2B call their sync once -- and what reaches
the update is the mean over ranks of the locally accumulated gradients."""
import pytest
import torch

from accum_dist_worker import K, STEPS, accum_worker
from dist_helpers import run_workers

WORLD = 2
PER_RANK_BATCH = 8


@pytest.fixture(scope="module")
def results():
    out = {}
    for strat in ["ddp", "gather_scatter", "allreduce"]:
        out[strat] = run_workers(accum_worker, WORLD, strat, PER_RANK_BATCH, 4.0)
        for r in range(WORLD):
            assert "error" not in out[strat][r], out[strat][r].get("error")
            assert out[strat][r]["iters"] == STEPS
    return out


def test_ddp_launches_each_bucket_once_per_optimizer_step(results):
    for r in range(WORLD):
        d = results["ddp"][r]
        assert d["n_buckets"] > 1
        assert d["bucket_launches"] == STEPS * d["n_buckets"]  # not K * STEPS * n_buckets
        assert d["buffer_syncs"] == STEPS  # the buffer broadcast: once per optimizer step


def test_replicas_are_identical(results):
    for strat in ["ddp", "gather_scatter", "allreduce"]:
        assert torch.equal(results[strat][0]["params"], results[strat][1]["params"]), strat
    assert results["ddp"][0]["consistent"] is True and results["ddp"][1]["consistent"] is True


def test_synced_grad_is_mean_of_locally_accumulated_grads(results):
    """Tolerance: the one test_dist_cpu.test_synced_grad_is_mean_of_local_grads uses."""
    for strat in ["ddp", "gather_scatter", "allreduce"]:
        d = results[strat][0]
        expected = (results[strat][0]["local"] + results[strat][1]["local"]) / WORLD
        assert torch.allclose(d["grads0"], expected, rtol=1e-5, atol=1e-7), strat
        assert not torch.allclose(d["grads0"], results[strat][0]["local"], rtol=1e-3, atol=1e-6)


def test_strategies_sync_once_per_optimizer_step_and_agree_with_ddp(results):
    """Tolerance: the one test_dist_cpu.test_strategies_agree uses."""
    a = results["ddp"][0]["params"]
    for strat in ["gather_scatter", "allreduce"]:
        for r in range(WORLD):
            assert results[strat][r]["syncs"] == STEPS  # not K * STEPS
        assert torch.allclose(results[strat][0]["params"], a, rtol=1e-5, atol=1e-6), strat
    assert K == 2
