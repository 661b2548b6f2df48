"""CPU oracle of the no-decay flag of the fused update launch (csrc/kernels/optim.hip: bit 8 of an
updating work item's kind word, bit 0 of the fourth field of a LAMB norms item), on top of
tests/update_oracle.py, tests/adamw_oracle.py and tests/lamb_oracle.py, which stay as they are
(``update_oracle.run_items`` refuses a kind it does not know, the flagged ones among them).

The flag means: this item's elements take the launch's rule with wd = 0 and nothing else changes.
So a table is split into its unflagged items, run with the launch's ``wd``, and its flagged items
with the flag stripped, run with ``wd = 0`` on the state the first pass left. The items of a
table are disjoint, so the order of the two passes does not matter; what a launch does once
whatever its items (the counter, the completion signal, the staged schedule step) is applied by
the first pass only.
"""
import torch

import adamw_oracle as ao
import lamb_oracle as lo
import update_oracle as uo

NO_DECAY = 0x100
KIND = 0xff
UPDATING = (0, 1, 2, 3)


def flagged(it):
    return bool(int(it[0]) & NO_DECAY)


def strip(it):
    """The item without its flag."""
    return [int(it[0]) & KIND] + [int(v) for v in it[1:]]


def split(items):
    """(unflagged items, flagged items with the flag stripped). A flag on a kind that updates
    nothing (4, 5) or any other high bit is refused, as update_oracle refuses an unknown kind."""
    plain, masked = [], []
    for it in items:
        k = int(it[0])
        if k & ~(KIND | NO_DECAY) or (flagged(it) and (k & KIND) not in UPDATING):
            raise ValueError(f"unknown item kind 0x{k:x}")
        (masked if flagged(it) else plain).append(strip(it))
    return plain, masked


def run_items(items, descs, p, g, buf, hyper, mem=None, shadow=None, slot=None, skip=0,
              counter=None, done=None, signal=None, sched=None, **kw):
    """``update_oracle.run_items`` of a table that may carry the flag (same arguments, same
    result)."""
    plain, masked = split(items)
    o = uo.run_items(plain, descs, p, g, buf, hyper, mem=mem, shadow=shadow, slot=slot, skip=skip,
                     counter=counter, done=done, signal=signal, sched=sched, **kw)
    if not masked:
        return o
    # the second pass reads the same step of the schedule and stages nothing again
    o2 = uo.run_items(masked, descs, o["p"], o["g"], o["buf"],
                      dict(hyper, wd=0.0, sched_advance=0), mem=o["mem"], shadow=o["shadow"],
                      slot=o["slot"], skip=skip, sched=sched, **kw)
    for k in ("p", "g", "buf", "mem", "shadow", "slot"):
        o[k] = o2[k]
    return o


def element_mask(items, n, descs=()):
    """bool [n]: the arena elements that a flagged elementwise item (kinds 0, 2, 3) owns."""
    m = torch.zeros(n, dtype=torch.bool)
    for it in items:
        kind, a, cnt, c = strip(it)
        if flagged(it) and kind in (0, 2, 3):
            off = a + (int(descs[c][0]) if kind == 2 else 0)
            m[off:off + cnt] = True
    return m


def adamw_ref(p, g, m, v, hp, masked, **kw):
    """``adamw_oracle.adamw_ref`` over flat tensors with ``wd = 0`` where ``masked`` (bool)."""
    a = ao.adamw_ref(p, g, m, v, hp, **kw)
    b = ao.adamw_ref(p, g, m, v, dict(hp, wd=0.0), **kw)
    return tuple(torch.where(masked, y, x) for x, y in zip(a, b))


def adamw_abs(p, g, m, v, hp, masked):
    """``adamw_oracle.adamw_abs`` with lw = 0 where ``masked``: dict of tensors (la stays a
    float)."""
    T = ao.adamw_abs(p, g, m, v, hp)
    T["lw"] = torch.where(masked, 0.0, torch.full(p.shape, float(T["lw"]), dtype=torch.float64))
    return T


def lamb_ref(p, g, m, v, hp, masked, **kw):
    """``lamb_oracle.lamb_ref`` of ONE tensor, with ``wd = 0`` when it is ``masked`` (bool)."""
    return lo.lamb_ref(p, g, m, v, dict(hp, wd=0.0) if masked else hp, **kw)


def lamb_abs(p, g, m, v, hp, masked):
    return lo.lamb_abs(p, g, m, v, dict(hp, wd=0.0) if masked else hp)
