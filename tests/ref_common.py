"""What the float64 references (tests/*_ref.py) share: the rounding constants, the bit-level bf16 arithmetic and the one
`worst_ratio` every kernel suite is judged by.  numpy only.  Not a test module: tests/test_kernel_harness.py tests it.  A
change here moves what every GPU suite accepts.
"""
import numpy as np

EPS32 = 2.0 ** -24               # one rounding to float32
EPS64 = 2.0 ** -53               # ... to float64
FLOOR = 2.0 ** -126              # added to bounds so that nothing hinges on denormals
BF16_REL = 2.0 ** -8             # half a bf16 spacing, relative
F, F64 = np.float32, np.float64
MODE_F32, MODE_BF16, MODE_F32X3 = 0, 1, 2          # DVAE_MODE_* of include/dvae_hip.h
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2


def g(k):
    """k fp32 roundings compounded."""
    return k * EPS32 / (1.0 - k * EPS32)


def bf16(x):
    """Round-to-nearest-even bf16 of fp32 values, as fp32."""
    u = np.ascontiguousarray(x, F).view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).astype(np.uint32).view(F)


def bf16_trunc(x):
    """bf16 of fp32 values by dropping the low 16 bits, as fp32."""
    return (np.ascontiguousarray(x, F).view(np.uint32) & 0xFFFF0000).astype(np.uint32).view(F)


def split3(x):
    """x == x1 + x2 + x3 exactly, three bf16 planes (fp32x3): x1 = rne(x), x2 = rne(x - x1), x3 = x - x1 - x2."""
    x = np.asarray(x, F)
    x1 = bf16(x)
    x2 = bf16(x - x1)
    return x1, x2, bf16(x - x1 - x2)


def fma(a, b, c):
    """a * b + c with one rounding to fp32 (the product of two fp32 values is exact in float64)."""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F)


def worst_ratio(got, ref, tol, inf_tol_unheld=False):
    """max |got - ref| / tol and where (a flat index); (0.0, -1) for empty input.  A value, a reference or a ratio that is
    not finite, or a NaN bound, counts as infinitely wrong.  So does a +inf bound, unless `inf_tol_unheld`: then nothing is
    held there (ratio 0)."""
    ref = np.asarray(ref, F64)
    if ref.size == 0:
        return 0.0, -1
    got, tol = np.asarray(got, F64), np.broadcast_to(np.asarray(tol, F64), ref.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - ref) / tol
    unheld = np.isposinf(tol) if inf_tol_unheld else False
    r = np.where(unheld, 0.0, r)
    r = np.where(np.isfinite(got) & np.isfinite(ref) & ~np.isnan(tol) & (unheld | np.isfinite(tol)) & ~np.isnan(r), r, np.inf)
    i = int(np.argmax(r))
    return float(r.reshape(-1)[i]), i
