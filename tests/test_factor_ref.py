"""The float64 restatement of the factor penalty (tests/factor_ref.py) on the CPU: its statistics
against the latent report's restatement, the identity with the joint total correlation, the closed-form gradients against
torch's float64 autograd and central differences, the duplicated style rows, the planted cases, and the plumbing (header,
binding, command-line errors)."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import factor_ref as R  # noqa: E402
import latents_ref as LR  # noqa: E402
from ref_common import F64  # noqa: E402


def model_case(seed, Bh, S, Cn, lv_lo=-3.0, lv_hi=1.0):
    """float64 z, mu, lv [2 Bh, S + Cn] with the model's structure: rows b and Bh + b share style posterior and sample"""
    rs = np.random.RandomState(seed)
    N, D = 2 * Bh, S + Cn
    mu, lv, eps = rs.randn(N, D), rs.uniform(lv_lo, lv_hi, (N, D)), rs.randn(N, D)
    mu[Bh:, :S], lv[Bh:, :S], eps[Bh:, :S] = mu[:Bh, :S], lv[:Bh, :S], eps[:Bh, :S]
    return mu + np.exp(0.5 * lv) * eps, mu, lv


# ------------------------------------------------------------------------------------------ against the latent report
@pytest.mark.parametrize("Bh,S,Cn", [(1, 1, 1), (3, 2, 4), (33, 4, 28)])
def test_statistics_are_the_latent_reports(Bh, S, Cn):
    rs = np.random.RandomState(Bh)
    N, D = 2 * Bh, S + Cn
    mu, lv, eps = rs.randn(N, D), rs.uniform(-3, 1, (N, D)), rs.randn(N, D)
    rep = LR.report(mu, lv, eps, np.zeros(N, np.int32), S, dtype=F64)
    z, mu_t, _, _ = rep["tables"]
    f = R.forward(z, mu_t, lv, S, 0.7, 0.3)
    s = dict(zip(R.STAT_NAMES, f["stats"]))
    tol = 1e-11 * (1 + np.abs(f["L"]).max())
    assert np.abs(f["L"] - rep["L_all"]).max() <= tol
    assert abs(s["tc_style"] - rep["style"]["tc"]) <= tol and abs(s["tc_content"] - rep["content"]["tc"]) <= tol
    assert abs(s["shared"] - rep["shared"]) <= tol and abs(s["mi"] - rep["joint"]["mi"]) <= tol
    # an identity of the definitions: the three penalised terms are the joint total correlation
    assert abs(s["tc_style"] + s["tc_content"] + s["shared"] - rep["joint"]["tc"]) <= tol
    assert abs(s["penalty"] - (0.7 * (s["tc_style"] + s["tc_content"]) + 0.3 * s["shared"])) <= 1e-15 * (1 + abs(s["penalty"]))


# ----------------------------------------------------------------------------------------------------- the gradients
def torch_penalty(z, mu, lv, S, w_tc, w_sh):
    """the restated forward in torch float64 (autograd)"""
    N, D = z.shape
    t = -0.5 * (R.LOG_2PI + lv[None] + (z[:, None, :] - mu[None]) ** 2 * torch.exp(-lv)[None])
    lnN = math.log(N)
    Ld = torch.logsumexp(t, dim=1) - lnN
    Ls, Lc = torch.logsumexp(t[..., :S].sum(-1), dim=1) - lnN, torch.logsumexp(t[..., S:].sum(-1), dim=1) - lnN
    Lj = torch.logsumexp(t.sum(-1), dim=1) - lnN
    tcs, tcc = (Ls - Ld[:, :S].sum(1)).mean(), (Lc - Ld[:, S:].sum(1)).mean()
    sh = (Lj - Ls - Lc).mean()
    return w_tc * (tcs + tcc) + w_sh * sh, (tcs, tcc, sh)


@pytest.mark.parametrize("w_tc,w_sh", [(1.5, 0.75), (0.0, 2.0), (1.0, 0.0), (1.0, 1.0)])
@pytest.mark.parametrize("Bh,S,Cn", [(1, 1, 1), (3, 2, 4), (9, 4, 6)])
def test_closed_forms_against_autograd_and_differences(Bh, S, Cn, w_tc, w_sh):
    z, mu, lv = model_case(7 + Bh, Bh, S, Cn)
    tz, tm, tl = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (z, mu, lv))
    pen, parts = torch_penalty(tz, tm, tl, S, w_tc, w_sh)
    pen.backward()
    f = R.forward(z, mu, lv, S, w_tc, w_sh)
    assert abs(float(pen.detach()) - f["stats"][4]) <= 1e-12 * (1 + abs(f["stats"][4]))
    for got, want in zip(f["stats"][:3], parts):
        assert abs(got - float(want.detach())) <= 1e-12 * (1 + abs(got))
    grads = R.gradients(z, mu, lv, S, w_tc, w_sh)
    for name, g_, ag in zip(("dz", "dmu", "dlv"), grads, (tz.grad, tm.grad, tl.grad)):
        scale = np.abs(ag.numpy()).max() + 1e-300
        assert np.abs(g_ - ag.numpy()).max() <= 1e-11 * scale, name
    # central differences on a handful of elements of each tensor
    rs = np.random.RandomState(3)
    h = 1e-6
    for k, name in enumerate(("z", "mu", "lv")):
        for _ in range(6):
            i, d = rs.randint(2 * Bh), rs.randint(S + Cn)
            args = [z.copy(), mu.copy(), lv.copy()]
            args[k][i, d] += h
            up = R.forward(*args, S, w_tc, w_sh)["stats"][4]
            args[k][i, d] -= 2 * h
            dn = R.forward(*args, S, w_tc, w_sh)["stats"][4]
            fd = (up - dn) / (2 * h)
            assert abs(fd - grads[k][i, d]) <= 1e-6 * (1 + np.abs(grads[k]).max()), (name, i, d, fd, grads[k][i, d])


def test_duplicated_style_rows():
    """Rows b and Bh + b carry the same style posterior and sample.  The penalty takes the rows as they are (2 Bh columns,
    duplicates included): with the two halves' content made equal as well, row b and row Bh + b are the same point and every
    gradient of the pair is equal; with different content, the gradients that reach the style columns differ in general but
    swap when the halves are swapped."""
    Bh, S, Cn = 4, 2, 3
    z, mu, lv = model_case(11, Bh, S, Cn)
    z2, mu2, lv2 = (np.concatenate([v[:Bh], v[:Bh]]) for v in (z, mu, lv))
    for g_ in R.gradients(z2, mu2, lv2, S, 1.5, 0.75):
        assert np.abs(g_[:Bh] - g_[Bh:]).max() <= 1e-13 * (1 + np.abs(g_).max())
    swap = np.concatenate([np.arange(Bh, 2 * Bh), np.arange(Bh)])
    a = R.gradients(z, mu, lv, S, 1.5, 0.75)
    b = R.gradients(z[swap], mu[swap], lv[swap], S, 1.5, 0.75)
    for x, y in zip(a, b):
        assert np.abs(x[swap] - y).max() <= 1e-12 * (1 + np.abs(x).max())
    fa, fb = R.forward(z, mu, lv, S, 1.5, 0.75), R.forward(z[swap], mu[swap], lv[swap], S, 1.5, 0.75)
    assert np.abs(fa["stats"] - fb["stats"]).max() <= 1e-12 * (1 + np.abs(fa["stats"]).max())
    # the duplicate is a column like any other: a style dimension's LSE always holds at least its two copies
    N = 2 * Bh
    assert np.all(fa["L"][:, :S] >= fa["t"][np.arange(N), np.arange(N), :S] + math.log(2.0) - 1e-12)


# ---------------------------------------------------------------------------------------------------- planted cases
def planted(seed, N=512, rho=0.0, sigma=0.5):
    """D = 2, S = 1: mu ~ N(0, [[1, rho], [rho, 1]]), posterior standard deviation sigma"""
    r = np.random.default_rng(seed)
    mu = r.standard_normal((N, 2)) @ np.linalg.cholesky(np.array([[1.0, rho], [rho, 1.0]])).T
    lv = np.full((N, 2), 2.0 * math.log(sigma))
    return mu + sigma * r.standard_normal((N, 2)), mu, lv


def test_independent_samples_and_a_planted_correlation():
    ind = [R.forward(*planted(s), 1)["stats"] for s in range(3)]
    cor = [R.forward(*planted(s, rho=0.8), 1)["stats"] for s in range(3)]
    for s in ind:
        # one dimension per block: the blocks' total correlations vanish identically; the minibatch estimator's known
        # positive bias on `shared` at N = 512 in two dimensions is a few hundredths of a nat
        assert abs(s[0]) <= 1e-12 and abs(s[1]) <= 1e-12
        assert -0.01 <= s[2] <= 0.08, s[2]
    # the Gaussian's mutual information between the two aggregate coordinates: -1/2 ln(1 - rho'^2), rho' = rho / (1 + sigma^2)
    want = -0.5 * math.log(1.0 - (0.8 / 1.25) ** 2)
    for s, s0 in zip(cor, ind):
        assert s[2] > s0[2] + 0.15 and abs(s[2] - want) <= 0.1, (s[2], want)


def test_following_the_gradient_lowers_shared():
    z, mu, lv = planted(0, N=128, rho=0.8)
    first = R.forward(z, mu, lv, 1, 0.0, 1.0)["stats"][2]
    vals = [first]
    for _ in range(5):
        dz, dmu, dlv = R.gradients(z, mu, lv, 1, 0.0, 1.0)
        z, mu, lv = z - 20.0 * dz, mu - 20.0 * dmu, lv - 20.0 * dlv
        vals.append(R.forward(z, mu, lv, 1, 0.0, 1.0)["stats"][2])
    assert all(b < a for a, b in zip(vals, vals[1:])), vals
    assert vals[-1] < first - 0.01, vals


# ------------------------------------------------------------------------------------------------ bounds and plumbing
def test_bounds_are_finite_and_small_where_the_data_allow():
    c = R.kernel_case(3, 2, 4, far=False)
    f = R.forward(c["z"], c["mu"], c["lv"], 2, *R.WEIGHTS)
    tau = R.tau_table(c["z"], c["mu"], c["lv"], 2, f["t"])
    BL = R.L_bound(f["t"], tau, f["L"])
    assert np.isfinite(BL).all() and (BL <= 1e-3 * (1 + np.abs(f["L"]))).all()
    for b, g_ in zip(R.gradient_bounds(c["z"], c["mu"], c["lv"], 2, *R.WEIGHTS, f["t"], tau, f["L"], BL),
                     R.gradients(c["z"], c["mu"], c["lv"], 2, *R.WEIGHTS)):
        assert np.isfinite(b).all() and (b > 0).all() and np.median(b) <= 1e-3 * np.abs(g_).max()
    # fp32 arithmetic on the same formulas stays inside them: a walk in numpy fp32 (not the kernel's order, the same counts)
    far = R.kernel_case(3, 2, 4, far=True)
    ff = R.forward(far["z"], far["mu"], far["lv"], 2)
    assert np.isfinite(R.L_bound(ff["t"], R.tau_table(far["z"], far["mu"], far["lv"], 2, ff["t"]), ff["L"])).all()


def test_kernel_cases_keep_the_models_structure():
    for Bh, S, Cn in R.SHAPES:
        c = R.kernel_case(Bh, S, Cn)
        assert c["z"].shape == (2 * Bh, S + Cn) and c["lv"].min() >= -8 and c["lv"].max() <= 2
        assert np.array_equal(c["mu"][:Bh, :S], c["mu"][Bh:, :S]) and np.array_equal(c["lv"][:Bh, :S], c["lv"][Bh:, :S])
    assert (65, 16, 48) in R.SHAPES and (32, 4, 28) in R.SHAPES


def test_header_and_binding_declare_the_entry_points():
    from dvae_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dvae_hip.h")).read()
    for name in ("dvae_factor_ws_bytes", "dvae_factor_fwd", "dvae_factor_bwd"):
        assert re.search(r"\b" + name + r"\(", hdr) and name in _lib.SIGNATURES
    assert int(re.search(r"#define DVAE_FACTOR_MAX_N (\d+)", hdr).group(1)) == _lib.FACTOR_MAX_N == R.MAX_N
    assert int(re.search(r"#define DVAE_LATENT_MAX_D (\d+)", hdr).group(1)) == _lib.LATENT_MAX_D == R.MAX_D
    n_args = lambda name: len(re.search(name + r"\(([^;]*)\);", hdr).group(1).split(","))
    for name in ("dvae_factor_fwd", "dvae_factor_bwd"):
        assert n_args(name) == len(_lib.SIGNATURES[name][1]), name
