"""The float64 reference of the gradient-norm kernels (csrc/elem.hip: grad_sumsq_kernel, grad_clip_finalize_kernel) and of
the clipped / guarded Adam step (dvae_adam_flat_dev_clip), with the bounds the kernels are held to.  Not a test module:
tests/test_grad_clip_ref.py proves the reference against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam and the bounds
against an fp32 restatement on the CPU, tests/test_hip_grad_clip.py holds the kernels to both.  A change here moves what
the GPU tests accept: the formula is clip_grad_norm_'s, the bounds are derived below, neither follows what some code computes.

The formula (clip_ref)
----------------------
    norm = gs * sqrt(sum g^2)                      gs = grad_scale: the norm of the gradient Adam consumes
    coef = min(1, max_norm / (norm + 1e-6))        clip_grad_norm_, its 1e-6 included
    eff  = gs * coef                               what Adam multiplies the gradient by in place of gs
    the step is skipped (p, m, v, t keep their values) when sum g^2 is not finite and the guard is up.
The square of a finite float32 is exact in float64 and n * FLT_MAX^2 ~ 1e85 does not overflow it, so the sum is not finite
exactly when some element is not.

The bounds
----------
eps32 = 2^-24 is one rounding to float32 (relative, for a normal result), eps64 = 2^-53 one to float64.
  norm:  |norm - ref| <= 2^-23 ref.  The kernel adds n exact squares in float64 in SOME order: the sum is off by at most
         n eps64 relative (every partial sum is at most the total, all terms being >= 0), the root halves that, the root
         and the product with gs add one eps64 each, and the store rounds once to float32: eps32 + (n/2 + 2) eps64, which
         is below 2 eps32 = 2^-23 for every n < 2^29.
  eff:   |eff - gs max_norm / (ref_norm + 1e-6)| <= 4 eps32 of that value, where the step is clipped.  The kernel forms the
         quotient and the product in float64 from its float64 norm and rounds once (eps32 + (n/2 + 5) eps64); the budget
         of four roundings also admits an implementation that goes on in float32 from the stored norm (clip_f32 with
         round_each=True: the norm, the sum with 1e-6, the quotient, the product — four roundings), so the bound does not
         prescribe where the doubles end.
         Where coef clamps to 1 there is no bound but equality: eff == gs bit for bit.
Both carry a floor of 2^-149 (half the spacing of float32 denormals, doubled): a coefficient of 1e-39 is a denormal.
"""
import math

import numpy as np

from ref_common import EPS32  # noqa: F401

NORM_REL = 2.0 ** -23
EFF_REL = 4 * EPS32
DENORM_FLOOR = 2.0 ** -149
CLIP_EPS = 1e-6                      # clip_grad_norm_'s


def sum_squares(g) -> float:
    """sum g^2 of float32 (or float64) values in float64, exactly rounded (math.fsum); inf / nan when an element is."""
    sq = np.asarray(g, dtype=np.float64) ** 2
    if not np.isfinite(sq).all():
        return float("nan") if np.isnan(sq).any() else float("inf")
    return math.fsum(sq.tolist()) if sq.size <= (1 << 16) else math.fsum(
        math.fsum(c.tolist()) for c in np.array_split(sq, 64))        # fsum of 64 fsums: 64 eps64 at most, far inside every bound


def clip_ref(g, gs: float, max_norm: float, sumsq: float = None):
    """(norm, coef, eff, nonfinite) in float64 from the gradient, the gradient scale and max_norm as the device holds them.
    `sumsq`: sum_squares(g) when the caller already has it."""
    gs, max_norm = float(gs), float(max_norm)
    s = sum_squares(g) if sumsq is None else float(sumsq)
    nonfinite = not math.isfinite(s)
    norm = gs * math.sqrt(s)
    ratio = max_norm / (norm + CLIP_EPS)             # inf / inf: NaN
    coef = ratio if ratio < 1.0 else 1.0             # a NaN ratio does not clip
    return norm, coef, gs * coef, nonfinite


def norm_tol(ref_norm: float) -> float:
    return NORM_REL * abs(ref_norm) + DENORM_FLOOR


def eff_tol(ref_eff: float) -> float:
    return EFF_REL * abs(ref_eff) + DENORM_FLOOR


def clipped_adam_step_ref(p, g, m, v, t, lr, b1, b2, eps, gs, max_norm, guard=True, eff=None):
    """One clipped / guarded step in float64: (p', m', v', t', info).  t counts the steps TAKEN: a skipped step leaves it,
    and p, m, v, where they are.  `eff`: use this scale (the kernel's own float32 one) in place of the reference's."""
    from adam_ref import adam_step_ref, bias_corrections
    norm, coef, ref_eff, nonfinite = clip_ref(g, gs, max_norm)
    info = {"norm": norm, "coef": coef, "eff": ref_eff, "nonfinite": nonfinite, "skipped": nonfinite and guard,
            "clipped": (not (nonfinite and guard)) and coef < 1.0}
    if info["skipped"]:
        return (np.asarray(p, np.float64), np.asarray(m, np.float64), np.asarray(v, np.float64), t, info)
    t = t + 1
    p2, m2, v2, _ = adam_step_ref(p, g, m, v, lr, b1, b2, eps, ref_eff if eff is None else eff, *bias_corrections(b1, b2, t))
    return p2, m2, v2, t, info


def clip_f32(g, gs, max_norm, round_each=False):
    """The finalize kernel's statements in numpy: squares added in float64 one after the other (np.cumsum: the worst order
    the bound allows), then either float64 throughout with one rounding per store (the kernel), or — round_each — float32 from the
    stored norm on.  Returns (norm, coef, eff) as float32."""
    F = np.float32
    s = float(np.cumsum(np.asarray(g, dtype=np.float64) ** 2)[-1])
    gs, max_norm = F(gs), F(max_norm)
    if round_each:
        with np.errstate(over="ignore"):
            norm = F(float(gs) * math.sqrt(s))
            ratio = max_norm / F(norm + F(CLIP_EPS))
        coef = ratio if ratio < 1 else F(1)
        return norm, F(coef), F(gs * coef)
    norm = float(gs) * math.sqrt(s)
    ratio = float(max_norm) / (norm + CLIP_EPS)
    coef = ratio if ratio < 1.0 else 1.0
    with np.errstate(over="ignore"):
        return F(norm), F(coef), F(float(gs) * coef)
