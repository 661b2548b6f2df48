"""Gradient accumulation in the deterministic-statistics build (run as a subprocess of
tests/test_gpu_accum_deterministic.py with DDP_AMD_DETERMINISTIC=1; prints one JSON line).
VGG-11, batch 8, 64 samples; every comparison is torch.equal.

    python tests/accum_probe.py sum     # arena gradient after 3 accumulate-only micro-steps ==
                                        #   the in-order fp32 sum of the three gradients alone
    python tests/accum_probe.py paths   # eager == captured, K = 2 and 3; == the hand-made step
    python tests/accum_probe.py k1      # accum_steps=1 is the step that was there before
    python tests/accum_probe.py ddp     # pipelined step (all-reduce / sharded plan) == TrainStep
    python tests/accum_probe.py guard   # gradient clipping and LARS: eager == captured; the norm
    python tests/accum_probe.py tail    # the leftover step and the eager loop == made by hand
    python tests/accum_probe.py loop1   # the captured K = 1 loop with a partial last batch == by hand
    python tests/accum_probe.py digest  # a SHA-256 of the end state per configuration: run in two
                                        #   checkouts, the outputs must be equal key for key
"""
import copy
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
B, N = 8, 64
HP = dict(lr=0.01, momentum=0.9, weight_decay=1e-4)


def _setup():
    import torch
    import ddp_amd
    assert ddp_amd.native().deterministic(), \
        "DDP_AMD_DETERMINISTIC=1 must load the deterministic build"
    return torch


class Rig:
    """One model + optimizer + loader with a start state every run returns to."""

    def __init__(self, base, opt_cls=None, ddp=False, n=N, **opt_kw):
        import torch
        from ddp_amd.data import DeviceLoader, SyntheticCIFAR10
        from ddp_amd.optim import FusedSGD
        self.model = copy.deepcopy(base)
        self.inner = self.model
        if ddp:
            from ddp_amd.parallel import DistributedDataParallel, RcclCommunicator
            self.model = DistributedDataParallel(
                self.model, RcclCommunicator(0, 1, 0, self_comm=False), bucket_cap_mb=256.0,
                first_bucket_cap_mb=256.0)
        self.opt = (opt_cls or FusedSGD)(self.model.parameters(), **dict(HP, **opt_kw))
        self.ld = DeviceLoader(SyntheticCIFAR10(True, n=n), B, "cuda")
        self.arena = self.opt.arena
        self.snap = (self.arena.data.clone(), self.opt.momentum_buffer.clone())
        torch.cuda.synchronize()

    def restore(self):
        import torch
        self.arena.data.copy_(self.snap[0])
        self.opt.momentum_buffer.copy_(self.snap[1])
        self.ld.cursor.zero_()
        self.arena.grad.zero_()
        if self.opt.schedule is not None:
            self.opt.set_lr_step(0)
        for sp in self.inner.fused_plan():
            sp._packed_version = None
            sp.maybe_pack()
        torch.cuda.synchronize()

    def state(self):
        """Masters, momentum, every bf16 operand copy and the cursor, after a synchronize."""
        import torch
        torch.cuda.synchronize()
        ops = []
        for sp in self.inner.fused_plan():
            for t in (sp.wc, getattr(sp, "wt", None)):
                if t is not None:
                    ops.append(t.clone())
        return {"p": self.arena.data.clone(), "buf": self.opt.momentum_buffer.clone(), "ops": ops,
                "cursor": int(self.ld.cursor)}

    def run(self, fn, steps=2):
        self.restore()
        for _ in range(steps):
            fn()
        return self.state()


def same(a, b):
    import torch
    return (torch.equal(a["p"], b["p"]) and torch.equal(a["buf"], b["buf"])
            and a["cursor"] == b["cursor"] and len(a["ops"]) == len(b["ops"])
            and all(torch.equal(x, y) for x, y in zip(a["ops"], b["ops"])))


def _base():
    import torch
    from ddp_amd.models import VGG11
    torch.manual_seed(31)
    return VGG11().cuda()


def _step(rig, K=1, cls=None, **kw):
    from ddp_amd.engine import CrossEntropyLoss, TrainStep
    return (cls or TrainStep)(rig.model, rig.opt, CrossEntropyLoss(), rig.ld, accum_steps=K, **kw)


def sum_case():
    torch = _setup()
    rig = Rig(_base())
    st = _step(rig, 3)
    st._body()  # builds the fused plan
    rig.restore()
    for j in range(3):
        st._accumulate(j)
    torch.cuda.synchronize()
    acc = rig.arena.grad.clone()
    singles = []
    for j in range(3):
        rig.restore()
        st._accumulate(j)
        torch.cuda.synchronize()
        singles.append(rig.arena.grad.clone())
    want = singles[0].clone().add_(singles[1]).add_(singles[2])
    bad = torch.nonzero(acc != want).flatten()
    offs = list(rig.arena.offsets)
    params = sorted({max(i for i, o in enumerate(offs) if o <= int(k))
                     for k in bad[:2000].tolist()})
    return {"nonzero": bool(float(acc.norm()) > 0) and all(float(s.norm()) > 0 for s in singles),
            "distinct": not torch.equal(singles[0], singles[1]),
            "sum_is_in_order_fp32_sum": torch.equal(acc, want),
            "differing_params": params[:20], "differing": int(bad.numel())}


def paths_case():
    torch = _setup()
    base = _base()
    res = {}
    for K in (2, 3):
        rig = Rig(base)
        st = _step(rig, K)
        res[f"K{K}/opt_in_bwd"] = bool(st.opt_in_bwd)
        eager = rig.run(st._body)
        res[f"K{K}/moved"] = not torch.equal(eager["p"], rig.snap[0])
        res[f"K{K}/cursor"] = eager["cursor"] == 2 * K
        res[f"K{K}/eager_repeatable"] = same(eager, rig.run(st._body))
        st.warmup(1)
        st.capture()
        res[f"K{K}/captured_equals_eager"] = same(eager, rig.run(st.step))
        res[f"K{K}/grad_clear"] = float(rig.arena.grad.abs().max()) == 0.0

        # the same two optimizer steps made by hand from the pieces: K accumulate-only
        # micro-steps, then the plain whole-arena update with float32(1 / K) and the cursor
        def by_hand():
            for j in range(K):
                st._accumulate(j)
            scale = float(torch.tensor(1.0 / K, dtype=torch.float32))
            rig.opt.grad_scale_factor = scale
            try:
                rig.opt.step(zero_grad=True, counter=rig.ld.cursor_advance(K))
            finally:
                rig.opt.grad_scale_factor = 1.0
        res[f"K{K}/by_hand_equals_eager"] = same(eager, rig.run(by_hand))
    return res


def k1_case():
    torch = _setup()
    from ddp_amd.engine import CrossEntropyLoss, TrainStep
    base = _base()
    out = []
    for explicit in (True, False):
        rig = Rig(base)
        st = (_step(rig, 1) if explicit
              else TrainStep(rig.model, rig.opt, CrossEntropyLoss(), rig.ld))
        st.warmup(2)  # (the first step of a model builds its plans: capture after the second)
        st.capture()
        out.append(rig.run(st.step))
    return {"moved": out[0]["cursor"] == 2, "k1_equals_default": same(out[0], out[1])}


def ddp_case():
    torch = _setup()
    from ddp_amd.engine import SegmentedDDPStep
    base = _base()
    K = 2
    rig = Rig(base)
    ref_step = _step(rig, K)
    ref_step.warmup(1)
    ref_step.capture()
    ref = rig.run(ref_step.step)
    res = {"moved": not torch.equal(ref["p"], rig.snap[0]) and ref["cursor"] == 2 * K}
    # diagnostic, not asserted: the same comparison without accumulation (the cut step against
    # the uncut step as they were before)
    r1 = Rig(base)
    s1 = _step(r1, 1)
    s1.opt_in_bwd = False
    p1 = r1.run(s1._body)
    d1 = Rig(base, ddp=True)
    c1 = _step(d1, 1, cls=SegmentedDDPStep, split=[3, 6])
    res["diag_k1_cut_equals_uncut"] = torch.equal(d1.run(c1._body)["p"], p1["p"])
    d1.model.close()
    for upd in ("allreduce", "shard16"):
        r = Rig(base, ddp=True)
        st = _step(r, K, cls=SegmentedDDPStep, split=[3, 6], update=upd)
        st.WAIT_TIMEOUT_S = 20.0
        e = r.run(st._body)
        st.warmup(1)
        st.capture()
        g = r.run(st.step)
        st.check_error()
        for name, got in (("eager", e), ("captured", g)):
            res[f"{upd}/{name}/p"] = torch.equal(got["p"], ref["p"])
            res[f"{upd}/{name}/buf"] = torch.equal(got["buf"], ref["buf"])
            res[f"{upd}/{name}/cursor"] = got["cursor"] == ref["cursor"]
        res[f"{upd}/grad_clear"] = float(r.arena.grad.abs().max()) == 0.0
        r.model.close()
    return res


def guard_case():
    torch = _setup()
    from ddp_amd.optim import LARS
    base = _base()
    K = 2
    res = {}
    # the accumulated gradient of the first step, from accumulate-only micro-steps
    rig = Rig(base, max_grad_norm=1e-3)
    st = _step(rig, K)
    res["guard/opt_in_bwd"] = bool(st.opt_in_bwd)
    st._body()
    rig.restore()
    for j in range(K):
        st._accumulate(j)
    torch.cuda.synchronize()
    g = rig.arena.grad.clone()
    a = rig.arena
    want = math.sqrt(sum(float((g[o:o + n].double() * 0.5).pow(2).sum())
                         for o, n in zip(a.offsets, a.numels)))
    e = rig.run(st._body, steps=1)
    got = float(rig.opt.grad_norm())
    res["guard/norm"], res["guard/norm_want"] = got, want
    res["guard/n_chunks"] = int(rig.opt._n_chunks)
    res["guard/clipped"] = float(rig.opt.clip_coef()) < 1.0
    e2 = rig.run(st._body)
    st.warmup(1)
    st.capture()
    res["guard/captured_equals_eager"] = same(e2, rig.run(st.step))
    res["guard/norm_replayed"] = float(rig.opt.grad_norm())
    res["guard/moved"] = not torch.equal(e["p"], rig.snap[0])
    rig = Rig(base, opt_cls=LARS, trust_coefficient=0.02)
    st = _step(rig, K)
    res["lars/opt_in_bwd"] = bool(st.opt_in_bwd)
    e = rig.run(st._body)
    st.warmup(1)
    st.capture()
    res["lars/captured_equals_eager"] = same(e, rig.run(st.step))
    res["lars/moved"] = not torch.equal(e["p"], rig.snap[0])
    return res


def _f32(v):
    import torch
    return float(torch.tensor(v, dtype=torch.float32))


def tail_case():
    """The leftover step of an accumulated epoch (TrainStep.tail_step on a list: two full
    batches and a partial one of 4, m = 3) and the eager loop train_model(accum_steps=2) over
    3 batches (groups of 2 and 1), each against the same thing made by hand: plain backward
    passes into the arena, then ONE opt.step with grad_scale float32(1 / m)."""
    torch = _setup()
    from ddp_amd.engine import CrossEntropyLoss, SegmentedDDPStep
    from ddp_amd.engine.trainer import train_model
    base = _base()
    res = {}
    rig = Rig(base)
    st = _step(rig, 3)
    st._body()  # builds the fused plan
    sizes = [(0, B), (B, B), (2 * B, 4)]

    def batches(r):
        return [r.ld.batch(s, n) for s, n in sizes]

    got = rig.run(lambda: st.tail_step(batches(rig)), steps=1)
    res["tail/moved"] = not torch.equal(got["p"], rig.snap[0])
    res["tail/grad_clear"] = float(rig.arena.grad.abs().max()) == 0.0
    res["tail/scale_restored"] = rig.opt.grad_scale_factor == 1.0
    one = torch.ones((), device="cuda")
    acc = torch.zeros((), device="cuda")

    def by_hand():
        for x, y in batches(rig):
            rig.model.forward_loss(x, y, acc=acc).backward(one)
        rig.opt.grad_scale_factor = _f32(1.0 / 3)
        try:
            rig.opt.step(zero_grad=True)
        finally:
            rig.opt.grad_scale_factor = 1.0
    res["tail/equals_by_hand"] = same(got, rig.run(by_hand, steps=1))

    def wrong_scale():  # the check can fail: the same step at 1 / K' with K' = 2
        for x, y in batches(rig):
            rig.model.forward_loss(x, y, acc=acc).backward(one)
        rig.opt.grad_scale_factor = 0.5
        try:
            rig.opt.step(zero_grad=True)
        finally:
            rig.opt.grad_scale_factor = 1.0
    res["tail/differs_from_wrong_scale"] = not same(got, rig.run(wrong_scale, steps=1))
    # the same list through the pipelined step's tail_step (all-reduce plan, world 1)
    r = Rig(base, ddp=True)
    seg = _step(r, 3, cls=SegmentedDDPStep, split=[3, 6])
    seg._body()
    g2 = r.run(lambda: seg.tail_step(batches(r)), steps=1)
    res["tail/segmented_equals_train_step"] = (torch.equal(g2["p"], got["p"])
                                                and torch.equal(g2["buf"], got["buf"]))
    r.model.close()

    # eager loop on the GPU: groups of 2 and 1 out of 3 loader batches
    crit = CrossEntropyLoss()
    rig.ld.max_batches = 3
    recs = []

    class Sink:
        def log(self, **kw):
            recs.append(kw["accum"])
    loop = rig.run(lambda: train_model(rig.model, rig.ld, rig.opt, crit, 0, "cuda",
                                       log=lambda s: None, metrics=Sink(), accum_steps=2), steps=1)
    res["eager/accum_fields"] = recs == [2, 1]
    res["eager/scale_restored"] = rig.opt.grad_scale_factor == 1.0

    def loop_by_hand():
        bs = list(rig.ld)
        for group in (bs[:2], bs[2:]):
            rig.opt.zero_grad()
            for x, y in group:
                crit(rig.model(x), y).backward()
            rig.opt.grad_scale_factor = _f32(1.0 / len(group))
            try:
                rig.opt.step()
            finally:
                rig.opt.grad_scale_factor = 1.0
    res["eager/equals_by_hand"] = same(loop, rig.run(loop_by_hand, steps=1))
    res["eager/moved"] = not torch.equal(loop["p"], rig.snap[0])
    return res


def _sched(opt):
    """The cosine schedule of tests/test_gpu_accum.py."""
    from ddp_amd.optim.schedule import LRSchedule
    opt.set_schedule(LRSchedule(0.01, 64, warmup_steps=2, decay="cosine"))


class Sink:
    def __init__(self):
        self.recs = []

    def log(self, **kw):
        self.recs.append(kw)

    def timeless(self):
        return [sorted((k, v) for k, v in r.items() if k != "ns") for r in self.recs]


def loop1_case():
    """train_model_graph with K = 1 over 60 samples at batch 8 (7 replays and an eager step on
    the partial batch of 4) with the default TrainStep (SGD in the backward) and a schedule,
    against the same eight steps made by hand."""
    torch = _setup()
    from ddp_amd.engine import CrossEntropyLoss, TrainStep
    from ddp_amd.engine.trainer import train_model_graph
    rig = Rig(_base(), n=60)
    _sched(rig.opt)
    st = TrainStep(rig.model, rig.opt, CrossEntropyLoss(), rig.ld)
    res = {"opt_in_bwd": bool(st.opt_in_bwd), "batches": len(rig.ld) == 8}
    st.warmup(2)
    st.capture()
    sink, stats = Sink(), {}
    got = rig.run(lambda: stats.update(train_model_graph(st, rig.ld, 0, log=lambda s: None,
                                                         metrics=sink)), steps=1)
    res["grad_clear"] = float(rig.arena.grad.abs().max()) == 0.0
    res["records"] = len(sink.recs) == 8 and [r["batch"] for r in sink.recs] == list(range(8))
    res["no_accum_key"] = all("accum" not in r for r in sink.recs)
    res["iters"] = len(stats["iter_ns"]) == 8
    res["graph_replays"] = stats["graph_replays"] == 7
    res["cursor"] = got["cursor"] == 7
    res["lr_step"] = rig.opt.lr_step_device() == 8 and rig.opt.lr_step == 8
    res["lr_values"] = [r["lr"] for r in sink.recs] == [rig.opt.schedule.lr_at(k)
                                                        for k in range(8)]
    res["moved"] = not torch.equal(got["p"], rig.snap[0])

    def by_hand():
        for _ in range(7):
            st._body()
        st.tail_step(*rig.ld.batch(56, 4))
    res["equals_by_hand"] = same(got, rig.run(by_hand, steps=1))
    res["by_hand_lr_step"] = rig.opt.lr_step_device() == 8 and rig.opt.lr_step == 8
    return res


def _digest(rig, fn, st=None, steps=2, extra=list):
    """SHA-256 over masters, momentum, every operand copy, the cursor, the device's schedule
    step and the raw bits of the popped loss meter after ``steps`` calls of ``fn`` from the
    restored start state (``extra()``: further values, read afterwards, by their repr). The
    digest of everything but the meter, and the meter's bits, also go to stderr: the head
    kernel adds one partial loss per 4 rows to the meter with a float atomic, so from the second
    micro-batch on the meter's last bit depends on which block of a batch of 8 adds first."""
    import hashlib
    import struct
    import torch
    rig.restore()
    if st is not None:
        st.pop_loss()
    for _ in range(steps):
        fn()
    state = rig.state()
    h = hashlib.sha256()
    for t in [state["p"], state["buf"]] + state["ops"]:
        h.update(t.contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes())
    h.update(struct.pack("<qq", state["cursor"], rig.opt.lr_step_device()))
    h.update(repr(extra()).encode())
    meter = struct.pack("<f", st.pop_loss()) if st is not None else b""
    print("state", h.hexdigest(), "meter", meter.hex(), file=sys.stderr)
    h.update(meter)
    return h.hexdigest()


def digest_case():
    """One digest per configuration; uses only names that the tree before the step routines
    were unified has too, so the same file runs in both."""
    _setup()
    from ddp_amd.engine import CrossEntropyLoss, SegmentedDDPStep
    from ddp_amd.engine.trainer import train_model, train_model_graph
    from ddp_amd.optim import LARS
    base = _base()
    res = {}

    def rig_of(**kw):
        rig = Rig(base, **kw)
        _sched(rig.opt)
        return rig

    def captured(name, rig, K, **kw):
        st = _step(rig, K, **kw)
        st.warmup(2)
        st.capture()
        res[name] = _digest(rig, st.step, st)
        return st

    st = captured("train/K1/in_bwd", rig_of(), 1)
    assert st.opt_in_bwd
    os.environ["DDP_AMD_SGD_IN_BWD"] = "0"
    try:
        st = captured("train/K1/no_in_bwd", rig_of(), 1)
        assert not st.opt_in_bwd
    finally:
        del os.environ["DDP_AMD_SGD_IN_BWD"]
    captured("train/K3", rig_of(), 3)
    for K in (1, 2):
        for upd in ("allreduce", "shard16"):
            rig = rig_of(ddp=True)
            st = _step(rig, K, cls=SegmentedDDPStep, split=[3, 6], emulate=1, update=upd)
            st.WAIT_TIMEOUT_S = 20.0
            st.warmup(2)
            st.capture()
            res[f"segmented/K{K}/{upd}"] = _digest(rig, st.step, st)
            st.check_error()
            rig.model.close()
    captured("train/K2/clip", rig_of(max_grad_norm=1e-3), 2)
    captured("train/K2/lars", rig_of(opt_cls=LARS, trust_coefficient=0.02), 2)

    rig = rig_of()
    st = _step(rig, 1)
    st.warmup(2)
    res["tail/partial4"] = _digest(rig, lambda: st.tail_step(*rig.ld.batch(0, 4)), st)
    rig = rig_of()
    st = _step(rig, 3)
    st.warmup(1)
    sizes = [(0, B), (B, B), (2 * B, 4)]
    res["tail/list"] = _digest(
        rig, lambda: st.tail_step([rig.ld.batch(s, n) for s, n in sizes]), st)

    crit = CrossEntropyLoss()
    for K in (1, 2):
        rig = rig_of()
        _step(rig, 1).warmup(1)  # builds the fused plan
        rig.ld.max_batches = 3
        sink = Sink()
        res[f"eager_loop/K{K}"] = _digest(
            rig, lambda: train_model(rig.model, rig.ld, rig.opt, crit, 0, "cuda",
                                     log=lambda s: None, metrics=sink, accum_steps=K),
            steps=1, extra=sink.timeless)
    for K in (1, 3):
        rig = rig_of(n=60)
        st = _step(rig, K)
        st.warmup(2)
        st.capture()
        sink = Sink()
        res[f"graph_loop/K{K}"] = _digest(
            rig, lambda: train_model_graph(st, rig.ld, 0, log=lambda s: None, metrics=sink,
                                           accum_steps=K),
            st, steps=1, extra=sink.timeless)
    return res


def main():
    res = {"sum": sum_case, "paths": paths_case, "k1": k1_case, "ddp": ddp_case,
           "guard": guard_case, "tail": tail_case, "loop1": loop1_case,
           "digest": digest_case}[sys.argv[1]]()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
