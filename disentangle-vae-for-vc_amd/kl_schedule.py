"""The KL weight as a pure host function of the optimiser's step count, and the free-bits vector.

`KLSchedule.weight_at(k, epoch, kl_cof)`: the weight of the step that runs when `k` optimiser steps have been taken
(`FlatAdam.t` before the step; the very first step has k = 0) in epoch `epoch` (1-based; only "double" looks at it).
Nothing here touches the device: the trainer copies the value into the `coef` buffer that the loss kernels read
(ops.LossGVAE2SchedFn), so a schedule never re-captures the step's graph, and a run resumed at step k continues with the
values of the uninterrupted run because the position is the step count itself.

    constant    kl_cof
    linear      start + (kl_cof - start) k / steps for k < steps, kl_cof from k = steps on
    cyclical    Fu et al. 2019: `steps` is cut into `cycles` equal cycles (a cycle may be a fractional number of steps: the
                position inside it is (k cycles mod steps) / steps, in integers); inside a cycle the weight goes linearly
                from start to kl_cof over the first `ratio` of it and holds; kl_cof from k = steps on
    double      the reference's update_kl() (model/disentangled_vae.py:346-347): start in epoch 1, doubled once per epoch,
                capped at kl_cof: min(start 2^(epoch - 1), kl_cof)
"""
from __future__ import annotations

import math

KINDS = ("constant", "linear", "cyclical", "double")
PARAM_KEYS = ("kind", "start", "steps", "cycles", "ratio", "free_bits")


class KLSchedule:
    def __init__(self, kind, start=0.0, steps=0, cycles=4, ratio=0.5, free_bits=None):
        if kind not in KINDS:
            raise ValueError(f"KL schedule {kind!r}: one of {KINDS} (None: off)")
        start, ratio = float(start), float(ratio)
        if isinstance(steps, bool) or isinstance(cycles, bool) or int(steps) != steps or int(cycles) != cycles:
            raise ValueError("KL schedule: steps and cycles are whole numbers")
        steps, cycles = int(steps), int(cycles)
        if not math.isfinite(start) or start < 0.0:
            raise ValueError(f"KL schedule: start must be a finite weight >= 0, got {start}")
        if steps < 0:
            raise ValueError(f"KL schedule: steps must be >= 0, got {steps}")
        if kind in ("linear", "cyclical") and steps < 1:
            raise ValueError(f"KL schedule {kind!r}: steps must be >= 1 (the length of the ramp in optimiser steps)")
        if kind == "cyclical" and not (1 <= cycles <= steps):
            raise ValueError(f"KL schedule 'cyclical': 1 <= cycles <= steps, got cycles {cycles}, steps {steps}")
        if kind == "cyclical" and not (0.0 < ratio <= 1.0):
            raise ValueError(f"KL schedule 'cyclical': ratio must be in (0, 1], got {ratio}")
        if kind == "double" and not start > 0.0:
            raise ValueError("KL schedule 'double': start must be > 0 (it is doubled once per epoch)")
        self.kind, self.start, self.steps, self.cycles, self.ratio = kind, start, steps, cycles, ratio
        self.free_bits = None if free_bits is None else [float(v) for v in free_bits]       # expanded: one per dimension

    def weight_at(self, k, epoch=1, kl_cof=10.0):
        k, epoch, top = int(k), int(epoch), float(kl_cof)
        if k < 0 or epoch < 1:
            raise ValueError(f"KL schedule: step count {k} / epoch {epoch} out of range")
        if self.kind == "constant":
            return top
        if self.kind == "double":
            return min(self.start * 2.0 ** (epoch - 1), top) if epoch <= 1024 else top
        if k >= self.steps:
            return top
        if self.kind == "linear":
            return self.start + (top - self.start) * (k / self.steps)
        pos = ((k * self.cycles) % self.steps) / self.steps          # position inside the cycle, in [0, 1)
        return self.start + (top - self.start) * min(1.0, pos / self.ratio)

    def params(self):
        """What a checkpoint keeps and a resume compares: plain numbers and lists."""
        return {"kind": self.kind, "start": self.start, "steps": self.steps, "cycles": self.cycles, "ratio": self.ratio,
                "free_bits": None if self.free_bits is None else list(self.free_bits)}


def expand_free_bits(free_bits, S, Cn):
    """None, one float for every dimension, a pair (style, content) or a length-(S + Cn) sequence -> None or S + Cn floats in
    the [S | Cn] layout of q_z*_mu, nats per dimension."""
    if free_bits is None:
        return None
    D = int(S) + int(Cn)
    if isinstance(free_bits, (int, float)) and not isinstance(free_bits, bool):
        vals = [float(free_bits)] * D
    else:
        vals = [float(v) for v in free_bits]
        if len(vals) == 2 and D != 2:
            vals = [vals[0]] * int(S) + [vals[1]] * int(Cn)
        elif len(vals) != D:
            raise ValueError(f"free_bits: one float, a (style, content) pair or {D} values, got {len(vals)}")
    if not all(math.isfinite(v) and v >= 0.0 for v in vals):
        raise ValueError("free_bits: finite values >= 0 (nats per dimension)")
    return vals
