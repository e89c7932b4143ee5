"""Float64 numpy restatement of the total-correlation / shared-information penalty of the train step (csrc/factor.hip,
ops.FactorPenaltyFn): the statistics, the three gradients as closed forms, the error bounds the kernels
are held to, and the shapes of the kernel tests.  Not a test module: tests/test_factor_ref.py and tests/test_hip_factor.py use
it.  Shapes: z / mu / lv [N, D], the S style columns first; L [N, D + 3]: the D dimensions, then style, content, joint.

    t_ijd = -1/2 (ln 2 pi + lv_jd + (z_id - mu_jd)^2 e^{-lv_jd}) = a_jd - h_jd (z_id - mu_jd)^2
    L_A(i) = log sum_j exp(sum_{d in A} t_ijd)
    tc_style = mean_i[(L_style - ln N) - sum_{d < S} (L_d - ln N)], tc_content likewise, shared = mean_i[L_joint - L_style -
    L_content + ln N], mi = mean_i[sum_d t_iid - (L_joint - ln N)], penalty = w_tc (tc_style + tc_content) + w_sh shared

The bounds, against float64 on the fp32 inputs (EPS32 = 2^-24 is one rounding, g(k) k of them compounded; expf and logf are
within 1 ulp = 2 EPS32, the HIP math library's documented error):

t           a = -(c32 + lv / 2): the constant's rounding and the sum's; h = expf(-lv) / 2: 2 roundings; dz = z - mu one, so two
            on dz^2, q = dz dz one; t = fma(-h, q, a) one:  tau = g(5) h dz^2 + EPS32 (|a| + c) + EPS32 |t|, times (1 + 2 EPS32).
block sums  the xor tree adds 64 lanes in 6 levels: tau_block = sum tau_d + g(6) sum |t_d|; joint = style + content adds one.
L, data     as latents_ref: L is convex with the softmax weights gamma as gradient; a perturbation |delta_j| <= tau_j moves it
            down by at most B0 = sum gamma_j tau_j and up by at most sum gamma_j tau_j exp(tau_j + B0), and never by more than
            the largest tau_j.
L, sums     term j of s = sum_j expf(x_j - M): the argument's rounding |x_j - M| EPS32 and the exponential's 2 EPS32, weighted
            by gamma_j (computed on the data, not bounded by an entropy); the additions: ceil(N / 4) + 3 roundings for a
            dimension, ceil(N / 64) + 6 for a block; logf within 1 ulp of ln s <= ln N; the last addition rounds L.  A flushed
            denormal exponential is below 2^-126 beside s >= 1: FLOOR per column.
statistics  float64 sums of fp32 L: the bound of a mean is the mean of the rows' bounds (each row's the sum of the bounds of
            the L it adds, own_i = joint_ii with its tau), plus the rounding of the result to fp32.
gradients   g_ijd = sum_A c_A p_A / N with p_A = expf(A_ij - L_A(i)): A_ij is off by tau_A, the L the kernel reads by B_L, the
            argument's rounding and the exponential add (|x| + 2) EPS32: p is off by p (exp(delta) - 1), and by 1 at most.  The three products,
            two additions, 1 / N and its use, and c_block = w_tc - w_sh: g(8) on sum_A |c_A| p_A / N.  r = 2 h dz: g(4);
            the factor of lv, fma(r / 2, dz, -1/2): g(6) on |r dz| / 2 and one rounding of itself.  A sum of N terms by fma adds
            g(N) on the sum of the ABSOLUTE terms; so every bound here is carried by sum |term|, never by the signed sum.
            A p, a g or a product below 2^-126 is flushed: FLOOR (1 + sum_A |c_A|) (1 + |factor|) per term.
"""
import math

import numpy as np

from ref_common import EPS32, F, F64, FLOOR, g

LOG_2PI = math.log(2.0 * math.pi)
HALF_LOG_2PI = 0.5 * LOG_2PI
MAX_D, MAX_N = 64, 1024            # DVAE_LATENT_MAX_D, DVAE_FACTOR_MAX_N
STAT_NAMES = ("tc_style", "tc_content", "shared", "mi", "penalty")


# ----------------------------------------------------------------------------------------------------------- forward
def table(z, mu, lv):
    """t [N, N, D] float64: t[i, j, d] = log q(z_id | x_j)"""
    z, mu, lv = (np.asarray(v, F64) for v in (z, mu, lv))
    return -0.5 * (LOG_2PI + lv[None] + (z[:, None, :] - mu[None]) ** 2 * np.exp(-lv)[None])


def sets(t, S):
    """t [N, N, D] -> [N, N, D + 3]: the dimensions, style, content, joint"""
    st, ct = t[..., :S].sum(-1), t[..., S:].sum(-1)
    return np.concatenate([t, st[..., None], ct[..., None], (st + ct)[..., None]], axis=-1)


def lse(x):
    """log-sum-exp over axis 1"""
    m = x.max(axis=1)
    return m + np.log(np.exp(x - m[:, None]).sum(axis=1))


def row_terms(L, own, S):
    """L [N, D + 3], own [N] = sum_d t_iid -> [N, 4]: the rows' terms of tc_style, tc_content, shared, mi"""
    L = np.asarray(L, F64)
    N, D = L.shape[0], L.shape[1] - 3
    lnN = math.log(N)
    Ld = L[:, :D] - lnN
    return np.stack([(L[:, D] - lnN) - Ld[:, :S].sum(1), (L[:, D + 1] - lnN) - Ld[:, S:].sum(1),
                     L[:, D + 2] - L[:, D] - L[:, D + 1] + lnN, np.asarray(own, F64) - (L[:, D + 2] - lnN)], axis=1)


def forward(z, mu, lv, S, w_tc=0.0, w_sh=0.0):
    """-> dict(L [N, D + 3], own [N], stats [5] in the order of STAT_NAMES, t = the [N, N, D + 3] table)"""
    t = sets(table(z, mu, lv), S)
    L = lse(t)
    N = L.shape[0]
    own = t[np.arange(N), np.arange(N), -1]
    s = row_terms(L, own, S).mean(0)
    stats = np.concatenate([s, [w_tc * (s[0] + s[1]) + w_sh * s[2]]])
    return dict(L=L, own=own, stats=stats, t=t)


# --------------------------------------------------------------------------------------------------------- gradients
def coefficients(D, S, w_tc, w_sh):
    """c_joint, c_block, c_d of the issue -> (c [D + 3] in the order of the table's last axis)"""
    return np.concatenate([np.full(D, -w_tc), [w_tc - w_sh, w_tc - w_sh, w_sh]]).astype(F64)


def _g_table(t, L, S, w_tc, w_sh, absolute=False):
    """g [N, N, D] (and, absolute, with |c_A| in place of c_A)"""
    N, D = t.shape[0], t.shape[2] - 3
    c = coefficients(D, S, w_tc, w_sh)
    if absolute:
        c = np.abs(c)
    p = np.exp(t - np.asarray(L, F64)[:, None, :])
    blk = np.concatenate([np.repeat(p[..., D:D + 1], S, axis=-1), np.repeat(p[..., D + 1:D + 2], D - S, axis=-1)], axis=-1)
    blk_c = np.concatenate([np.full(S, c[D]), np.full(D - S, c[D + 1])])
    return (c[D + 2] * p[..., D + 2:D + 3] + blk_c * blk + c[:D] * p[..., :D]) / N


def gradients(z, mu, lv, S, w_tc, w_sh, L=None):
    """the closed forms of d penalty / d (z, mu, lv), float64 -> (dz, dmu, dlv) [N, D].  L: the L to use (default: its own)"""
    z, mu, lv = (np.asarray(v, F64) for v in (z, mu, lv))
    t = sets(table(z, mu, lv), S)
    gt = _g_table(t, lse(t) if L is None else L, S, w_tc, w_sh)
    df = z[:, None, :] - mu[None]
    r = df * np.exp(-lv)[None]
    return (gt * -r).sum(1), (gt * r).sum(0), (gt * (-0.5 + 0.5 * r * df)).sum(0)


# ------------------------------------------------------------------------------------------------------------ bounds
def tau_table(z, mu, lv, S, t):
    """the bound of the kernel's fp32 t, style, content, joint against `t` -> [N, N, D + 3]"""
    z, mu, lv = (np.asarray(v, F64) for v in (z, mu, lv))
    D = z.shape[1]
    hq = 0.5 * np.exp(-lv)[None] * (z[:, None, :] - mu[None]) ** 2
    a = np.abs(0.5 * (LOG_2PI + lv))[None]
    td = np.abs(t[..., :D])
    tau = (g(5) * hq + EPS32 * (a + HALF_LOG_2PI) + EPS32 * td) * (1 + 2 * EPS32) + FLOOR
    ts = tau[..., :S].sum(-1) + g(6) * td[..., :S].sum(-1)
    tc = tau[..., S:].sum(-1) + g(6) * td[..., S:].sum(-1)
    tj = ts + tc + EPS32 * (np.abs(t[..., D + 2]) + ts + tc)
    return np.concatenate([tau, ts[..., None], tc[..., None], tj[..., None]], axis=-1)


def L_bound(t, tau, L):
    """the bound of every L [rows, D + 3] of rows against N = t.shape[1] columns (module docstring: data + sums)"""
    N, D = t.shape[1], t.shape[2] - 3
    with np.errstate(over="ignore", invalid="ignore"):
        gam = np.exp(t - L[:, None])
        b0 = (gam * tau).sum(axis=1)
        up = np.exp(t - L[:, None] + tau + b0[:, None]) * tau
        up = np.where(np.isfinite(up), up, np.inf).sum(axis=1)
    data = np.minimum(np.maximum(b0, up), tau.max(axis=1))
    args = (gam * (np.abs(t - t.max(axis=1)[:, None]) + tau)).sum(axis=1) * EPS32 + 2 * EPS32
    adds = np.concatenate([np.full(D, g(-(-N // 4) + 3)), np.full(3, g(-(-N // 64) + 6))])[None]
    sums = (args + adds) * (1 + 1e-3) + 2 * EPS32 * math.log(N) + EPS32 * (np.abs(L) + 1.0) + FLOOR * N
    return data + sums


def stats_bound(BL, tau_own, stats, S, w_tc, w_sh):
    """BL [N, D + 3], tau_own [N] (the joint tau of the diagonal) -> the bounds of the five statistics"""
    D = BL.shape[1] - 3
    rows = np.stack([BL[:, D] + BL[:, :S].sum(1), BL[:, D + 1] + BL[:, S:D].sum(1), BL[:, D:D + 3].sum(1),
                     tau_own + BL[:, D + 2]], axis=1)
    b = rows.mean(0) * (1 + 1e-6)
    b = np.concatenate([b, [abs(w_tc) * (b[0] + b[1]) + abs(w_sh) * b[2]]])
    return b + EPS32 * np.abs(np.asarray(stats, F64)) + FLOOR


def gradient_bounds(z, mu, lv, S, w_tc, w_sh, t, tau, L_used, BL):
    """bounds of dz, dmu, dlv [N, D] for a kernel that read `L_used` (each element within BL of the float64 L)"""
    z, mu, lv = (np.asarray(v, F64) for v in (z, mu, lv))
    N, D = z.shape
    c = np.abs(coefficients(D, S, w_tc, w_sh))
    p = np.exp(t - np.asarray(L_used, F64)[:, None, :])
    # p is off by exp(x + delta) - exp(x), x = A_ij - L_A(i); the kernel's p and the true one both lie in [0, 1] (L >= M >= A_ij
    # on the same bits), so no error exceeds 1
    x = t - np.asarray(L_used, F64)[:, None, :]
    delta = tau + BL[:, None, :] + (np.abs(x) + 2.0) * EPS32 * (1 + 1e-3)
    with np.errstate(over="ignore", under="ignore"):
        dp = np.where(delta < 1.0, p * np.expm1(np.minimum(delta, 1.0)), np.exp(np.minimum(x + delta, 0.0)) - p)
    dp = np.minimum(dp, 1.0)
    blk = lambda v: np.concatenate([np.repeat(v[..., D:D + 1], S, axis=-1), np.repeat(v[..., D + 1:D + 2], D - S, axis=-1)], axis=-1)
    blk_c = np.concatenate([np.full(S, c[D]), np.full(D - S, c[D + 1])])
    g_abs = (c[D + 2] * p[..., D + 2:D + 3] + blk_c * blk(p) + c[:D] * p[..., :D]) / N
    g_err = (c[D + 2] * dp[..., D + 2:D + 3] + blk_c * blk(dp) + c[:D] * dp[..., :D]) / N + g(8) * g_abs
    df = z[:, None, :] - mu[None]
    r = np.abs(df * np.exp(-lv)[None])
    f = -0.5 + 0.5 * r * np.abs(df)                 # r dz >= 0: |r| |dz| is r dz
    f_err = g(6) * 0.5 * r * np.abs(df) + EPS32 * np.abs(f)
    f = np.abs(f)
    one = 1 + 1e-6
    tz = g_abs * r
    # a p, a g or a term below 2^-126 is flushed to zero: FLOOR (1 + sum |c_A|) on g, times the factor, per term
    fl = FLOOR * (1.0 + c[D] + c[D + 2] + c[0])
    bz = ((g_err * r + g_abs * g(4) * r) * one + fl * (1 + r)).sum(1) + g(N) * tz.sum(1) + FLOOR
    bm = ((g_err * r + g_abs * g(4) * r) * one + fl * (1 + r)).sum(0) + g(N) * tz.sum(0) + FLOOR
    bl = ((g_err * f + g_abs * f_err) * one + fl * (1 + f)).sum(0) + g(N) * (g_abs * f).sum(0) + FLOOR
    return bz, bm, bl


# ------------------------------------------------------------------------------------- the shapes of the kernel tests
SHAPES = [(1, 1, 1), (1, 2, 2), (3, 2, 4), (32, 4, 28), (33, 4, 28), (65, 16, 48)]      # (Bh, S, Cn)
WEIGHTS = (1.5, 0.75)              # w_tc, w_sh of the kernel tests: c_block = 0.75


def kernel_case(Bh, S, Cn, far=True):
    """fp32 z, mu, lv [2 Bh, S + Cn] with the model's structure (rows b and Bh + b share the style posterior and sample),
    lv in [-8, 2]; row 0 of z lies far from every column, its own included; the last row's softmax is one-hot (its own
    column has lv = -8 everywhere and z on its mean, every other column lies 50 of ITS standard deviations away).
    far=False leaves the far row out: that row's softmax is decided by roundings (tau is of the order of 1e5 there), so with
    it the bounds of its dz and of every dmu, dlv it enters are finite but say little; without it they are tight.
    -> dict(z, mu, lv, far, hot)"""
    rs = np.random.RandomState(1000 * Bh + 37 * S + Cn)
    N, D = 2 * Bh, S + Cn
    mu = rs.randn(N, D)
    lv = rs.uniform(-8.0, 2.0, (N, D))
    eps = rs.randn(N, D)
    mu[Bh:, :S], lv[Bh:, :S], eps[Bh:, :S] = mu[:Bh, :S], lv[:Bh, :S], eps[:Bh, :S]
    hot = N - 1
    if N > 2:
        lv[hot] = -8.0
        eps[hot] = 0.0
        if Bh > 1:                                  # the style columns are shared with row Bh - 1: keep the structure
            lv[Bh - 1, :S] = -8.0
            eps[Bh - 1, :S] = 0.0
    z = mu + np.exp(0.5 * lv) * eps
    if N > 2:
        others = np.array([j for j in range(N) if j not in (hot, Bh - 1)])
        mu[hot, S:] = 50.0 * np.exp(0.5 * 2.0) + np.abs(mu[:, S:]).max() + np.arange(Cn)
        z[hot, S:] = mu[hot, S:]
        assert len(others)
    if far:
        z[0] = (np.abs(mu).max() + math.exp(1.0)) * 300.0 * np.where(np.arange(D) % 2, -1.0, 1.0)
    return dict(z=z.astype(F), mu=mu.astype(F), lv=lv.astype(F), far=0 if far else None, hot=hot if N > 2 else None)
