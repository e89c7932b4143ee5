"""The float64 reference of gradient clipping and the non-finite guard (tests/grad_clip_ref.py), proved without a GPU:
`clip_ref` followed by `adam_ref.adam_step_ref` is torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in float64, a gradient
that is not finite leaves a guarded step where it was, and the bounds the kernels are held to (tests/test_hip_grad_clip.py)
hold for an fp32 restatement of the finalize kernel in numpy."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from adam_ref import BETAS, EPS, LR, grad_mixture, params  # noqa: E402
from grad_clip_ref import (EFF_REL, NORM_REL, clip_f32, clip_ref, clipped_adam_step_ref, eff_tol, norm_tol,  # noqa: E402
                           sum_squares)


def _relclose(a, b, rel, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    bad = np.abs(a - b) > rel * np.abs(b)
    assert not bad.any(), (what, int(bad.sum()), a[bad][:3], b[bad][:3])


@pytest.mark.parametrize("max_norm", [50.0, 1e9], ids=["clipping", "not clipping"])
def test_reference_is_clip_grad_norm_then_torch_adam_in_float64(max_norm):
    n, (b1, b2) = 4096, BETAS
    p, m, v, t = params(1, n).astype(np.float64), np.zeros(n), np.zeros(n), 0
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([tp], lr=LR, betas=BETAS, eps=EPS)
    for step in range(1, 4):
        g = grad_mixture(20 + step, n)
        tp.grad = torch.from_numpy(g.astype(np.float64))
        total = torch.nn.utils.clip_grad_norm_([tp], max_norm)
        opt.step()
        p, m, v, t, info = clipped_adam_step_ref(p, g, m, v, t, LR, b1, b2, EPS, 1.0, max_norm)
        assert t == step and info["clipped"] == (max_norm < 1e9) and not info["skipped"]
        assert abs(info["norm"] - float(total)) <= 1e-13 * float(total)
        st = opt.state[tp]
        _relclose(p, tp.detach().numpy(), 1e-12, f"p at step {step}")
        _relclose(m, st["exp_avg"].numpy(), 1e-12, f"exp_avg at step {step}")
        _relclose(v, st["exp_avg_sq"].numpy(), 1e-12, f"exp_avg_sq at step {step}")


def test_reference_norm_is_the_scaled_gradients_norm():
    g = grad_mixture(5, 1000)
    a = clip_ref(g, 0.5, 10.0)
    b = clip_ref(0.5 * g.astype(np.float64), 1.0, 10.0)
    assert abs(a[0] - b[0]) <= 1e-15 * b[0] and abs(a[1] - b[1]) <= 1e-15 * b[1]
    assert abs(a[2] - 0.5 * b[2]) <= 1e-15 * b[2]
    assert clip_ref(np.zeros(8, np.float32), 1.0, 1.0)[:3] == (0.0, 1.0, 1.0)
    assert clip_ref(g, 0.5, math.inf)[1:3] == (1.0, 0.5)                    # inf: never clips, eff is gs itself


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_reference_skips_a_step_whose_gradient_is_not_finite(bad):
    n, (b1, b2) = 64, BETAS
    p, g = params(2, n), grad_mixture(3, n).copy()
    m, v = np.full(n, 0.01), np.full(n, 1e-4)
    g[17] = bad
    assert not math.isfinite(sum_squares(g))
    for max_norm in (1.0, math.inf):
        p2, m2, v2, t2, info = clipped_adam_step_ref(p, g, m, v, 5, LR, b1, b2, EPS, 1.0, max_norm)
        assert info["nonfinite"] and info["skipped"] and not info["clipped"] and t2 == 5
        assert np.array_equal(p2, p.astype(np.float64)) and np.array_equal(m2, m) and np.array_equal(v2, v)
        with np.errstate(invalid="ignore"):
            p2, m2, v2, t2, info = clipped_adam_step_ref(p, g, m, v, 5, LR, b1, b2, EPS, 1.0, max_norm, guard=False)
        assert info["nonfinite"] and not info["skipped"] and t2 == 6
        assert not np.isfinite(p2).all()                                     # the guard is what protects the weights


def test_huge_but_finite_gradients_are_clipped_not_skipped():
    g = np.array([3e38, -3e38, 3e38, -3e38], dtype=np.float32)
    norm, coef, eff, nonfinite = clip_ref(g, 1.0, 1.0)
    assert not nonfinite and norm > float(np.finfo(np.float32).max) and math.isfinite(norm)
    assert np.allclose(eff * g.astype(np.float64), [0.5, -0.5, 0.5, -0.5], rtol=1e-6)
    with np.errstate(over="ignore"):
        n32, c32, e32 = clip_f32(g, 1.0, 1.0)
    assert np.isinf(n32) and abs(float(e32) - eff) <= eff_tol(eff)            # eff is a float32 denormal: the floor term


@pytest.mark.parametrize("round_each", [False, True], ids=["float64, one rounding", "float32 from the norm on"])
@pytest.mark.parametrize("gs", [1.0, 0.5, 0.125])
def test_fp32_restatement_meets_the_bounds(gs, round_each):
    worst_n, worst_e = 0.0, 0.0
    for seed, n in enumerate([4, 2044, 2052, 6208, 100003]):
        g = grad_mixture(300 + seed, n)
        s = sum_squares(g)
        ref_norm = clip_ref(g, gs, math.inf, sumsq=s)[0]
        for k in (0.1, 0.5, 0.999, 2.0, math.inf):
            max_norm = np.float32(k * ref_norm)
            norm, coef, eff, _ = clip_ref(g, gs, max_norm, sumsq=s)
            n32, c32, e32 = clip_f32(g, gs, max_norm, round_each=round_each)
            worst_n = max(worst_n, abs(float(n32) - norm) / norm_tol(norm))
            if coef < 1.0:
                assert c32 < 1.0 or abs(coef - 1.0) < 4 * EFF_REL
                worst_e = max(worst_e, abs(float(e32) - eff) / eff_tol(eff))
            else:
                assert float(e32) == float(np.float32(gs)) and float(c32) == 1.0      # the clamp is exact
    print(f"fp32 restatement, gs={gs}, round_each={round_each}: worst error / bound: norm {worst_n:.3f} (bound {NORM_REL:.3g} "
          f"relative), eff {worst_e:.3f} (bound {EFF_REL:.3g} relative)")
    assert worst_n <= 1.0 and worst_e <= 1.0 and worst_e > 0.0
