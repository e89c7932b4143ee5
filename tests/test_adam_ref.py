"""The float64 reference of the Adam step kernels (csrc/elem.hip: adam_kernel, adam_dev_kernel), proved without a GPU.

`adam_step_ref` restates the kernels' formula in numpy float64.  Here it is held to torch.optim.Adam on float64
parameters (1e-12 relative on p, exp_avg and exp_avg_sq over 10 steps), and the distance between the Adam the device
runs — beta1, beta2, eps, lr and both bias corrections are float32 on the device — and the double-precision Adam of
torch is bounded.  The reference, the gradient mixture and the one-step rounding bounds live in tests/adam_ref.py (no test module), which
tests/test_hip_adam.py imports as well; the bounds are checked here on an fp32 restatement of the kernel in numpy.

The float32-hyperparameter gap (test_float32_hyperparameters_move_the_update_by_less_than_2e_5)
------------------------------------------------------------------------------------------------
With constant hyperparameters  m_t/bc1_t = sum_k w_k(b1) g_k  and  v_t/bc2_t = sum_k w_k(b2) g_k^2  are weighted means,
w_k(b) = (1-b) b^(t-k) / (1-b^t), sum_k w_k = 1.  Rounding b to float32 moves every weight by
    d ln w_k = db * [ -1/(1-b) + (t-k)/b + t b^(t-1)/(1-b^t) ],
and the first and the last term cancel up to O(t): the bracket lies in [-4.1, 6.0] for b1 = 0.9 and in [-4.5, 9.0] for
b2 = 0.999 while t <= 10.  float32(0.999) - 0.999 = 1.29e-8 (1.3e-5 relative in 1-b2) therefore moves v_t/bc2_t by at most
1.2e-7 relative and its root by 6e-8; at t = 1 not at all, the bias correction divides the same 1-b2 out again.  (It is NOT
6.5e-6 at t = 1 decaying afterwards: that figure forgets the bias correction.  The full 1.3e-5 / 2 is only approached
after thousands of steps, when bc2 -> 1 no longer follows 1-b2, and only for gradients whose magnitude changed within the
last ~1/(1-b2) steps.)  lr, bc1 and bc2s are each rounded once more (<= 6e-8 each), eps counts for nothing where
sqrt(v) > 100 eps.  That is 2.4e-7 in all for the denominator and the step size.
The numerator is different: the g_k are signed, so the weighted mean can cancel.  With kappa = sum_k w_k |g_k| / |sum_k w_k g_k|
(1 where all gradients of an element had one sign) the float32 beta1 (float32(0.9) - 0.9 = -2.4e-8) moves m_t/bc1_t by at
most 6.0 * 2.4e-8 * kappa = 1.43e-7 kappa relative.  So, for t <= 10 and sqrt(v) > 100 eps,
    |u32 - u64| / |u64|  <=  2.4e-7 + 1.43e-7 kappa,
which is below 2e-5 for kappa <= 100 and not otherwise: an element whose first moment cancelled to a thousandth of its
terms has a tiny update either way, and the two Adams disagree about it by 1e-4 of that tiny update.
Measured (10 steps, 4096 elements): median gap 7e-8; maximum over kappa <= 100: 7.5e-6 with log-uniform gradients and
8.2e-6 with the mixture (bound there: 1.5e-5); over all kappa 1.3e-4 (log-uniform, kappa about 1e3 there) and 4.4e-5
(mixture), always within the kappa bound above.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from adam_ref import (BETAS, EPS, EPS32, LR, adam_step_f32, adam_step_ref, bias_corrections, f32, grad_mixture,  # noqa: E402,F401
                      one_step_bounds, params, worst_ratio)


# ------------------------------------------------------------------ the reference is torch.optim.Adam
def _loguniform_grads(seed, n):
    rs = np.random.RandomState(seed)
    return 10.0 ** rs.uniform(-12.0, 3.0, n) * rs.choice([-1.0, 1.0], n)


def _relclose(a, b, rel, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    bad = np.abs(a - b) > rel * np.abs(b)
    assert not bad.any(), (what, int(bad.sum()), a[bad][:3], b[bad][:3])


@pytest.mark.parametrize("kind", ["loguniform", "mixture"])
def test_reference_is_torch_adam_in_float64(kind):
    n, (b1, b2) = 4096, BETAS
    p = params(1, n).astype(np.float64)
    m, v = np.zeros(n), np.zeros(n)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([tp], lr=LR, betas=BETAS, eps=EPS)
    for t in range(1, 11):
        g = _loguniform_grads(10 + t, n) if kind == "loguniform" else grad_mixture(10 + t, n).astype(np.float64)
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v, _ = adam_step_ref(p, g, m, v, LR, b1, b2, EPS, 1.0, *bias_corrections(b1, b2, t))
        st = opt.state[tp]
        _relclose(p, tp.detach().numpy(), 1e-12, f"p at step {t}")
        _relclose(m, st["exp_avg"].numpy(), 1e-12, f"exp_avg at step {t}")
        _relclose(v, st["exp_avg_sq"].numpy(), 1e-12, f"exp_avg_sq at step {t}")
    assert int(st["step"]) == 10


def test_reference_applies_grad_scale_to_the_gradient():
    n, (b1, b2) = 257, BETAS
    p, g = params(2, n), grad_mixture(3, n)
    m, v = np.abs(params(4, n)) * 0.1, np.abs(params(5, n)) * 0.01
    a = adam_step_ref(p, g, m, v, LR, b1, b2, EPS, 0.125, 0.19, 0.045)
    b = adam_step_ref(p, 0.125 * g.astype(np.float64), m, v, LR, b1, b2, EPS, 1.0, 0.19, 0.045)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------ float32 hyperparameters
def _weight_log_derivative_range(b, t):
    """Extremes over k = 1..t of  d ln w_k / db  for w_k = (1-b) b^(t-k) / (1-b^t)."""
    base = -1.0 / (1.0 - b) + t * b ** (t - 1) / (1.0 - b ** t)
    return base, base + (t - 1) / b


def hyperparameter_gap_bound(t, kappa, b1=BETAS[0], b2=BETAS[1]):
    """Relative distance of the update between float32-rounded and double hyperparameters after t steps (module docstring)."""
    c1 = max(abs(x) for x in _weight_log_derivative_range(b1, t)) * abs(f32(b1) - b1)
    c2 = max(abs(x) for x in _weight_log_derivative_range(b2, t)) * abs(f32(b2) - b2)
    rounded_once = 3 * EPS32                 # lr, bc1, bc2s
    eps_share = EPS32 / 100.0                # float32(eps) where eps is below 1/100 of the denominator
    return c1 * kappa + 0.5 * c2 + rounded_once + eps_share


@pytest.mark.parametrize("kind", ["loguniform", "mixture"])
def test_float32_hyperparameters_move_the_update_by_less_than_2e_5(kind):
    """The device's Adam (float32 betas, eps, lr and bias corrections) against the double one, update by update."""
    n, (b1, b2) = 4096, BETAS
    b1f, b2f, epsf, lrf = f32(b1), f32(b2), f32(EPS), f32(LR)
    pa = params(1, n).astype(np.float64)
    pb, ma, va, mb, vb, mabs = pa.copy(), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    worst_plain, worst_all, checked = 0.0, 0.0, 0
    for t in range(1, 11):
        g = _loguniform_grads(10 + t, n) if kind == "loguniform" else grad_mixture(10 + t, n).astype(np.float64)
        pa, ma, va, ua = adam_step_ref(pa, g, ma, va, LR, b1, b2, EPS, 1.0, *bias_corrections(b1, b2, t))
        bc1f, bc2sf = (f32(x) for x in bias_corrections(b1f, b2f, t))
        pb, mb, vb, ub = adam_step_ref(pb, g, mb, vb, lrf, b1f, b2f, epsf, 1.0, bc1f, bc2sf)
        mabs = mabs + (np.abs(g) - mabs) * (1.0 - b1)
        sel = (np.sqrt(va) > 100 * EPS) & (ma != 0)
        kappa = mabs[sel] / np.abs(ma[sel])
        gap = np.abs(ub[sel] - ua[sel]) / np.abs(ua[sel])
        bound = hyperparameter_gap_bound(t, kappa)
        assert (gap <= bound).all(), (t, float((gap / bound).max()))
        plain = kappa <= 100.0
        assert (bound[plain] < 2e-5).all()
        assert (gap[plain] < 2e-5).all(), (t, float(gap[plain].max()))
        worst_plain, worst_all = max(worst_plain, float(gap[plain].max())), max(worst_all, float(gap.max()))
        checked += int(plain.sum())
    print(f"float32-hyperparameter gap of the update, {kind}: {worst_plain:.3g} (kappa <= 100), {worst_all:.3g} (all)")
    assert checked > 5 * n            # the bound was held by most elements at most steps, not by a remnant
    assert worst_plain > 1e-8         # ... and the two runs did differ


# ------------------------------------------------------------------ the one-step bounds, on an fp32 restatement
@pytest.mark.parametrize("gs", [1.0, 0.125, 3.0])
@pytest.mark.parametrize("flipping", [False, True])
def test_fp32_restatement_meets_the_one_step_bounds(gs, flipping):
    n = 6208
    b1f, b2f = np.float32(BETAS[0]), np.float32(BETAS[1])
    p, m, v = params(1, n), np.zeros(n, np.float32), np.zeros(n, np.float32)
    worst = {"m": 0.0, "v": 0.0, "p": 0.0, "p_cancel": 0.0}
    for t in range(1, 21):
        g = grad_mixture(100 + t if flipping else 100, n)
        bc = [np.float32(x) for x in bias_corrections(float(b1f), float(b2f), t)]
        sc = (np.float32(LR), b1f, b2f, np.float32(EPS), np.float32(gs), *bc)
        with np.errstate(under="ignore"):
            p2, m2, v2 = adam_step_f32(p, g, m, v, *sc)
        b = one_step_bounds(p, g, m, v, *sc, cancel=True)
        for k, got, ref, tol in (("m", m2, "ref_m", "tol_m"), ("v", v2, "ref_v", "tol_v"), ("p", p2, "ref_p", "tol_p"),
                                 ("p_cancel", p2, "ref_p", "tol_p_cancel")):
            worst[k] = max(worst[k], worst_ratio(got, b[ref], b[tol])[0])
        p, m, v = p2, m2, v2
    print(f"fp32 restatement, gs={gs}, {'flipping' if flipping else 'fixed'} signs, worst error / bound: "
          + ", ".join(f"{k} {x:.3f}" for k, x in worst.items()))
    assert worst["m"] <= 1.0 and worst["v"] <= 1.0 and worst["p_cancel"] <= 1.0, worst
    if not flipping:                               # flipping signs: m' can cancel and the 12-rounding form need not hold
        assert worst["p"] <= 1.0, worst
