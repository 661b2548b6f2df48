"""Input block's fused weight gradient in the deterministic-statistics build (run as a subprocess
of tests/test_gpu_l0_wgrad.py with DDP_AMD_DETERMINISTIC=1; prints one JSON line).

The fused dz pass (conv_l0.hip l0_bwd_kernel<2>) maps tiles to blocks statically and sums its
block partials in one fixed order with plain stores, so two calls on the same inputs must give
bitwise-equal weight gradients.

    python tests/l0_wgrad_probe.py
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    import torch
    import ddp_amd
    from ddp_amd.ops.common import stat_replicas
    nat = ddp_amd.native()
    assert nat.deterministic(), "DDP_AMD_DETERMINISTIC=1 must load the deterministic build"
    from test_gpu_l0_wgrad import _block
    torch.manual_seed(3)
    # 4608 tiles on 4096 waves: accumulation across the tile loop and every block partial
    blk = _block(nat, 72, 32, 32, bias=True, nrep=stat_replicas())
    a = blk.fused(torch.zeros_like(blk.conv.weight, memory_format=torch.channels_last))
    b = blk.fused(torch.zeros_like(blk.conv.weight, memory_format=torch.channels_last))
    torch.cuda.synchronize()
    print(json.dumps({"equal": bool(torch.equal(a["dw"], b["dw"])),
                      "nonzero": float(a["dw"].abs().max()) > 0,
                      "finite": bool(torch.isfinite(a["dw"]).all())}))


if __name__ == "__main__":
    main()
