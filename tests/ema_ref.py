"""The float64 reference of the weight-average kernels (csrc/elem.hip: ema_tick_kernel, ema_update_kernel) and the bound one
fp32 update is held to.  Not a test module: tests/test_ema_ref.py proves the reference against the closed form of an
exponential moving average and against torch.optim.swa_utils, and the bound against an fp32 restatement on the CPU;
tests/test_hip_ema.py holds the kernels to both.  A change here moves what the GPU tests accept: the formula is the usual
EMA, the bound is derived below, neither follows what some code computes.

The formula
-----------
    tick (a step that is applied):   k <- k + 1
                                     d_k = min(decay, (1 + k) / (10 + k)) with warm-up, decay without      (the NEW k)
                                     w_k = 1 - d_k
    update:                          e <- e + w_k (p - e)          ==  d_k e + (1 - d_k) p
    a skipped step changes nothing: neither k, nor w, nor e.
`decay` is what the device holds: a float32.  d_k and w_k are evaluated in float64 from it; the kernel stores w_k rounded once
to float32, so |w - w_k| <= 2^-24 w_k (TICK_REL = 2^-23 leaves room for the double operations in front of the rounding).

The bound of one update (update_bounds)
---------------------------------------
The sweep is held to the float64 update fed the kernel's OWN float32 w, so that the tick's rounding (checked on its own) is not
counted twice.  eps32 = 2^-24 is one rounding to float32.  The kernel rounds twice:
    s  = fl(p - e)        = (p - e)(1 + d1)                         |d1| <= eps32   (exact when p and e are within a factor 2)
    e' = fl(w s + e)      = (w s + e)(1 + d2)                       |d2| <= eps32   (one rounding: an fma)
so with ref = e + w (p - e):
    e' - ref = w (p - e) d1 + ref d2 + w (p - e) d1 d2
    |e' - ref| <= eps32 (w |p - e| (1 + eps32) + |ref|)
plus the reference's own float64 roundings, 4 * 2^-53 (w |p - e| + |e|), and a floor of 2^-126 so that nothing hinges on
denormals (adam_ref.FLOOR, for the same reason).  Where p == e bit for bit there is no bound but equality: s = +0 and
w * 0 + e = e (tests/test_hip_ema.py asserts the bits).  An implementation that rounds the product before the sum (no fma)
is off by a further eps32 w |p - e|: ema_update_f32(fused=False) shows that this bound tells the two apart.
"""
import math

import numpy as np

from ref_common import EPS32, EPS64, FLOOR, worst_ratio  # noqa: F401

TICK_REL = 2.0 ** -23


def decay_at(decay, k: int, warmup: bool) -> float:
    """d_k in float64 from the float32 decay the device holds; k >= 1 is the number of the update (after the increment)."""
    d = float(np.float32(decay))
    return min(d, (1.0 + k) / (10.0 + k)) if warmup else d


def weight_at(decay, k: int, warmup: bool) -> float:
    """w_k = 1 - d_k in float64: what the tick stores, rounded once to float32, into ema_state[2]."""
    return 1.0 - decay_at(decay, k, warmup)


def tick_ref(k: int, decay, warmup: bool, skipped: bool = False):
    """(k', w', applied) of one tick from k updates so far; w' is None on a skipped step (ema_state[2] keeps its bits)."""
    if skipped:
        return k, None, 0
    return k + 1, weight_at(decay, k + 1, warmup), 1


def ema_update_ref(e, p, w) -> np.ndarray:
    """e + w (p - e) in float64, term by term as the kernel has it."""
    e, p = np.asarray(e, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return e + float(w) * (p - e)


def update_bounds(e, p, w):
    """Reference and rounding bound of ONE fp32 update from the float32 inputs with the float32 w the kernel holds.
    Returns {"ref", "tol"} (module docstring)."""
    e, p, w = np.asarray(e, dtype=np.float64), np.asarray(p, dtype=np.float64), float(w)
    ref = ema_update_ref(e, p, w)
    move = abs(w) * np.abs(p - e)
    tol = EPS32 * (move * (1.0 + EPS32) + np.abs(ref)) + 4.0 * EPS64 * (move + np.abs(e)) + FLOOR
    return {"ref": ref, "tol": tol}


def ema_update_f32(e, p, w, fused=True) -> np.ndarray:
    """The kernel's statements in numpy float32.  fused: the product w s is exact in float64 (24 x 24 bits) and the sum is
    rounded to float64, then to float32 — an fma up to a double rounding of 2^-53, which the bound's float64 term covers.
    Not fused: product and sum rounded to float32 one after the other."""
    F = np.float32
    e, p, w = np.asarray(e, dtype=F), np.asarray(p, dtype=F), F(w)
    s = (p - e).astype(F)
    if fused:
        return (float(w) * s.astype(np.float64) + e.astype(np.float64)).astype(F)
    return ((w * s).astype(F) + e).astype(F)


def closed_form(e0, ps, ds) -> np.ndarray:
    """e_K = (prod_j d_j) e_0 + sum_j (1 - d_j) (prod_{i > j} d_i) p_j in float64: ps[j], ds[j] belong to update j + 1."""
    e0 = np.asarray(e0, dtype=np.float64)
    out = math.prod(ds) * e0 if len(ds) else e0.copy()
    for j, (pj, dj) in enumerate(zip(ps, ds)):
        out = out + (1.0 - dj) * math.prod(ds[j + 1:]) * np.asarray(pj, dtype=np.float64)
    return out
