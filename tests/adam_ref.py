"""The float64 reference of the Adam step kernels (csrc/elem.hip: adam_kernel, adam_dev_kernel) and the rounding bounds
one fp32 step is held to.  Not a test module: tests/test_adam_ref.py proves the reference against torch.optim.Adam and the
bounds against an fp32 restatement on the CPU, tests/test_hip_adam.py holds the kernels to both.  A change here moves what
the GPU tests accept: the formula is the kernels', the bounds are derived below, neither follows what some code computes.

The one-step rounding bounds (one_step_bounds)
----------------------------------------------
eps32 = 2^-24, one rounding per fp32 operation, with or without FMA contraction, plus a floor of 2^-126 so that nothing
hinges on denormals:
    |m' - ref| <= 4 eps32 (|m| + |gs g|)         gs*g, the difference, the product with 1-b1, the sum
    |v' - ref| <= 4 eps32 ref                    (5 eps32 in the worst case when gs*g is inexact: gs*g counts twice)
    |p' - ref| <= eps32 |ref| + 12 eps32 |u|     the final rounding of p, and 12 roundings in u = (lr/bc1) m' / (sqrt(v')/bc2s + eps)
The last one counts m' as 4 roundings RELATIVE to m', which holds while m and gs*g do not cancel.  Where they do (m = -106,
g = 1e3: m' = 4.2 carries the absolute error of its terms, fifty times its own rounding) it does not, and the bound that
always holds carries the absolute bound of m' through the division instead:
    |p' - ref| <= eps32 |ref| + 8 eps32 |u| + (lr/bc1) * 4 eps32 (|m| + |gs g|) / (sqrt(v')/bc2s + eps)
(`tol_p_cancel`; never smaller than the first form).  The difference shows only where p itself is small: |u| <= ~lr, so
for |p| > 1e-3 the term eps32 |ref| covers either form.  An fp32 restatement of the kernel in numpy is checked against
both here: with one gradient sign per element the first form holds; with signs flipping between steps it is exceeded
(1.75 x) by one element-step of 124 160 (p = -3.9e-5, the m and g above) and the second form holds everywhere.
"""
import math

import numpy as np

from ref_common import EPS32, FLOOR, worst_ratio  # noqa: F401

# exact zeros, and magnitudes whose sqrt(v) is far below, near and far above eps = 1e-8
GRAD_VALUES = np.array([0.0, 1e-30, -1e-30, 1e-12, -1e-12, 1e-8, -1e-8, 1e-4, -1e-4, 1.0, -1.0, 1e3, -1e3], dtype=np.float32)
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8


def f32(x) -> float:
    """x rounded to float32, as a Python double."""
    return float(np.float32(x))


def grad_mixture(seed: int, n: int) -> np.ndarray:
    """n float32 gradients drawn uniformly from GRAD_VALUES."""
    return GRAD_VALUES[np.random.RandomState(seed).randint(0, len(GRAD_VALUES), n)]


def params(seed: int, n: int) -> np.ndarray:
    return np.random.RandomState(seed).uniform(-1.0, 1.0, n).astype(np.float32)


def bias_corrections(b1: float, b2: float, t: int):
    """(1 - b1^t, sqrt(1 - b2^t)) in double: what adam_tick_kernel stores (rounded to float32) from its float32 betas."""
    return 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)


def adam_step_ref(p, g, m, v, lr, b1, b2, eps, gs, bc1, bc2s):
    """One Adam step in float64, the kernels' formula term by term.  Returns (p', m', v', u) with p' = p - u."""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    lr, b1, b2, eps, gs, bc1, bc2s = (float(x) for x in (lr, b1, b2, eps, gs, bc1, bc2s))
    gr = gs * g
    m2 = m + (gr - m) * (1.0 - b1)
    v2 = b2 * v + (1.0 - b2) * gr * gr
    u = (lr / bc1) * m2 / (np.sqrt(v2) / bc2s + eps)
    return p - u, m2, v2, u


def one_step_bounds(p, g, m, v, lr, b1, b2, eps, gs, bc1, bc2s, cancel=False):
    """Reference and rounding bounds of ONE fp32 step from the float32 inputs (p, g, m, v) with the float32 scalars the
    kernel holds.  Returns a dict: ref_p, ref_m, ref_v, u, tol_p, tol_m, tol_v, and with `cancel` tol_p_cancel (module
    docstring)."""
    rp, rm, rv, u = adam_step_ref(p, g, m, v, lr, b1, b2, eps, gs, bc1, bc2s)
    tol_m = (4 * EPS32) * (np.abs(np.asarray(m, np.float64)) + np.abs(float(gs) * np.asarray(g, np.float64))) + FLOOR
    out = {"ref_p": rp, "ref_m": rm, "ref_v": rv, "u": u, "tol_m": tol_m, "tol_v": (4 * EPS32) * rv + FLOOR,
           "tol_p": EPS32 * np.abs(rp) + (12 * EPS32) * np.abs(u) + FLOOR}
    if cancel:
        den = np.sqrt(rv) / float(bc2s) + float(eps)
        tol_pc = EPS32 * np.abs(rp) + (8 * EPS32) * np.abs(u) + abs(float(lr) / float(bc1)) * tol_m / den + FLOOR
        out["tol_p_cancel"] = np.maximum(out["tol_p"], tol_pc)
    return out


def adam_step_f32(p, g, m, v, lr, b1, b2, eps, gs, bc1, bc2s):
    """The kernel's statements in numpy float32, one rounding per operation (no contraction)."""
    F = np.float32
    p, g, m, v = (np.asarray(x, dtype=F) for x in (p, g, m, v))
    lr, b1, b2, eps, gs, bc1, bc2s = (F(x) for x in (lr, b1, b2, eps, gs, bc1, bc2s))
    step_size = lr / bc1
    gr = g * gs
    m2 = m + (gr - m) * (F(1) - b1)
    v2 = v * b2 + (F(1) - b2) * gr * gr
    p2 = p - step_size * (m2 / (np.sqrt(v2) / bc2s + eps))
    return p2, m2, v2
