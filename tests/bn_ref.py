"""The float64 reference of the batch-norm kernels (csrc/bn.hip: the five entry points dvae_bn_stats_fwd,
dvae_bn_stats_finalize, dvae_bn_apply_fwd, dvae_bn_bwd, dvae_bn_bwd_from_y) and the rounding bounds one launch is held to.
Not a test module: tests/test_bn_ref.py proves the reference against torch.nn.BatchNorm1d in float64 and the bounds against
an fp32 restatement on the CPU, tests/test_hip_bn.py holds the kernels to both.  A change here moves what the GPU tests
accept: the formulas are the kernels', the bounds are derived below, neither follows what some code computes.

Group rule (include/dvae_hip.h): row r of the [R, C] matrix is in segment r % N and group (r % N) / (N/G); every group holds
cnt = (R/N) (N/G) rows.  Statistics are per (group, channel).

The bounds.  eps32 = 2^-24 is one fp32 rounding, eps64 = 2^-53 one fp64 rounding, g(k) = k eps32 / (1 - k eps32) is k
roundings compounded, FLOOR = 2^-126 keeps denormals out of every question.  Every bound is a function of float64
quantities computed from what the launch READ (the device's own fp32 mean, rstd, Z, s12 are inputs, not errors).

mean, rstd (tol_mean, tol_rstd)
    The kernels add fp64 terms: a thread adds the y (and the y^2, exact in fp64: 24 + 24 bits) of ROWS_PER_CHUNK/4 = 16
    rows, four row lanes are added in LDS (3 additions), sum_partials adds ceil(chunks/64) chunk partials per thread, then
    4 shuffle steps and 3 additions over the four waves: a partial passes through
        a = 16 + 3 + ceil(chunks/64) + 4 + 3            (tree_adds; 64 + 7 + ceil(chunks/64) from partials the host wrote:
                                                         numpy adds the 64 rows of a chunk in turn)
    additions, so  |S1' - S1| <= a eps64 sum|y|  and  |S2' - S2| <= a eps64 sum y^2  (all terms of S2 have one sign).
    mean = (float)(S1'/cnt):   |mean' - mean| <= eps32 |mean| + (a + 1 + 16) eps64 E|y|      (the division; 16 eps64 for
    the pairwise float64 sum of the reference itself).
    var' = S2'/cnt - m'^2, clamped at 0:  the error of S2'/cnt is (a+1) eps64 E[y^2], m' carries (a+1) eps64 E|y|, so m'^2
    is off by 2 |m| (a+1) eps64 E|y| + eps64 m^2 <= (2a + 3) eps64 E[y^2]  (|m| <= E|y| <= sqrt(E[y^2])), the subtraction
    rounds once more:   |var' - var| <= c eps64 E[y^2],   c = 3 (a + 1) + 2        (var_roundings; 86 up to 64 chunks).
    rstd = (float)(1/sqrt(var' + eps)): with d = c eps64 E[y^2] / (var + eps),
        |rstd' - rstd| <= rstd (eps32 + 4 eps64 + ((1 - d)^-1/2 - 1)),      (1 - d)^-1/2 - 1 = d/2 + O(d^2),
    i.e. one fp32 rounding plus the cancellation term  c 2^-53 E[y^2] / (var + eps) / 2  (exact form used so that the
    bound also holds where d is not small; for d >= 1 only 0 < rstd' <= eps^-1/2 is known, the bound is infinite).
    With kappa = mean^2/var, E[y^2]/(var + eps) <= 1 + kappa: the cancellation term stays below ONE fp32 rounding while
        1 + kappa < 2^30 / c = 1.2e7   (c = 86),   |mean|/std < 3.5e3;
    the model's activations reach |mean|/std <~ 1e3 after a conv (kappa = 1e6: at most 0.08 eps32 from this term).
running_mean, running_var (tol_running)
    Per group, in group order, in fp32:  r' = (1 - mom) r + mom (float)x,  x = the float64 mean, or the unbiased variance
    var cnt/(cnt - 1) (the biased one at cnt == 1).  (1 - mom) and its product with r are two roundings of the first term,
    (float)x and its product with mom two of the second, the sum one of both (an FMA saves one):
        tol' = |1 - mom| tol (1 + eps32) + g(3) (|(1 - mom) r| + |mom x|) + |mom| dx,
    dx = the fp64 error of x from above ((a+17) eps64 E|y|, or c eps64 E[y^2] cnt/(cnt-1)), tol = 0 before the first group.
z (tol_u, tol_z)
    u = (y - mean) rstd gamma + beta in fp32: the difference, two products (three roundings of A = |y - mean| rstd |gamma|)
    and the sum (one rounding of |u| <= A + |beta|; fused with the last product it saves one):
        |u' - u| <= g(4) (A + |beta|).
    act none / ReLU (1-Lipschitz, exact): the same for z.  With a residual one more rounding of |act(u)| + |residual|:
        |z' - z| <= g(5) (A + |beta| + |residual|).
    act tanh:  |z' - z| <= sech^2(max(|u| - tol_u, 0)) tol_u + TANHF_ROUNDINGS eps32 |tanh u|   (+ with a residual
    eps32 (|tanh u| + |residual|) and the compounding of both).  TANHF_ROUNDINGS: the device's tanhf is not documented by
    the project and no accuracy table of the math library is installed, so it was measured against
    float64 tanh over a dense sweep of [-10, 10]; the bound is twice the worst observed.
du, yhat (inside bwd_bounds)
    yhat = (y - mean) rstd: two roundings, |dyh| <= g(2) |yh|.  du = dz * act'(z): exact for act none / ReLU (a factor 0 or
    1); tanh: 1 - z^2 rounds z^2 and the difference, the product once more:
        |ddu| <= eps32 |dz| (z^2 + |1 - z^2|) + eps32 |du|        (NOT relative to du: 1 - z^2 cancels near saturation).
s1 = sum du, s2 = sum du yhat per (group, channel); dgamma += sum_g s2, dbeta += sum_g s1
    fp64 sums of the fp32 terms above (du yhat is exact in fp64), b = a - 1 + 17 additions as for the mean:
        |s1' - s1| <= sum ddu + b eps64 sum|du| + eps32 |s1|
        |s2' - s2| <= sum (|yh| ddu + g(2) |du yh|) + b eps64 sum|du yh| + eps32 |s2|
    each channel against its own sum.  dgamma' = old + (float)(sum_g s2) in fp32: the term errors of both groups, one
    rounding of the total and one of old + total; dbeta likewise.
dy (tol inside bwd_bounds)
    dy = gamma rstd (du - s1/cnt - yh s2/cnt) with the device's own fp32 s1, s2 (they are held to their own bounds above).
    1/cnt rounds once.  du passes two subtractions, gamma*rstd and the last product: 4 roundings (+ ddu); s1/cnt its product
    and those four, and 1/cnt: 6; yh s2/cnt: yh (2), two products, 1/cnt, one subtraction and the last two: 8.  So
        |dy' - dy| <= |gamma rstd| (g(8) (|du| + |s1|/cnt + |yh s2|/cnt) + ddu),
    a sum of absolute values: cancellation inside the bracket is covered, FMA contraction only removes roundings.
bf16 stores have no bound: they are the round-to-nearest-even of the fp32 value, compared bit for bit in the GPU tests.
"""
import functools

import numpy as np

import ref_common
from ref_common import ACT_NONE, ACT_RELU, ACT_TANH, EPS32, EPS64, F, F64, FLOOR, fma as _fma, g  # noqa: F401

ROWS_PER_CHUNK = 64                       # DVAE_BN_ROWS_PER_CHUNK of csrc/common.h
# Device tanhf against float64 tanh, |tanhf(x) - tanh(x)| / (eps32 |tanh(x)|): measured worst 2.4333 (at x = 0.634837687) over 40 000 001 evenly
# spaced x in [-10, 10] and 2^23 log-spaced |x| in [1e-6, 10] on the MI355X (scripts/probes/tanhf_sweep.hip; DESIGN.md
# section 5).  The sweep is a sample: the bound is twice that.
TANHF_MEASURED = 2.4333
TANHF_ROUNDINGS = 2.0 * TANHF_MEASURED


def groups(R, N, G):
    """Group of every row."""
    return (np.arange(R) % N) // (N // G)


def count(R, N, G):
    return (R // N) * (N // G)


def n_chunks(R):
    return (R + ROWS_PER_CHUNK - 1) // ROWS_PER_CHUNK


def tree_adds(R, from_partials=False):
    """fp64 additions one term passes through on its way into a statistic (module docstring)."""
    a = 3 + -(-n_chunks(R) // 64) + 4
    # from_partials: the host's own sums of a chunk's rows, which numpy adds in turn, take the place of the first stage
    return a + ROWS_PER_CHUNK if from_partials else a + ROWS_PER_CHUNK // 4 + 3


def var_roundings(R, from_partials=False):
    return 3 * (tree_adds(R, from_partials) + 1) + 2


def group_sum(x, R, N, G):
    """[G, C] sums of the rows of x [R, C] per group, float64."""
    x = np.asarray(x, F64)
    gi = groups(R, N, G)
    return np.stack([x[gi == k].sum(0) for k in range(G)])


def per_row(s, R, N, G):
    """[G, C] -> [R, C]: every row gets its group's value."""
    return np.asarray(s, F64)[groups(R, N, G)]


# ------------------------------------------------------------------ the operations, float64
def stats(y, N, G, eps):
    """mean[G, C], biased var[G, C], rstd[G, C] = 1/sqrt(var + eps), two-pass."""
    y = np.asarray(y, F64)
    R = y.shape[0]
    cnt = count(R, N, G)
    mean = group_sum(y, R, N, G) / cnt
    var = group_sum((y - per_row(mean, R, N, G)) ** 2, R, N, G) / cnt
    return mean, var, 1.0 / np.sqrt(var + float(eps))


def running(rm, rv, mean, var, cnt, momentum):
    """running_mean, running_var after one call: once per group in group order, unbiased variance (biased at cnt == 1,
    the kernel's rule: torch refuses one value per channel)."""
    rm, rv, mom = np.asarray(rm, F64).copy(), np.asarray(rv, F64).copy(), float(momentum)
    for k in range(mean.shape[0]):
        unb = var[k] * cnt / (cnt - 1.0) if cnt > 1 else var[k]
        rm = (1.0 - mom) * rm + mom * mean[k]
        rv = (1.0 - mom) * rv + mom * unb
    return rm, rv


def act_apply(u, act):
    return np.maximum(u, 0.0) if act == ACT_RELU else np.tanh(u) if act == ACT_TANH else u


def apply(y, mean, rstd, gamma, beta, residual, N, G, act):
    """(u, z): u = (y - mean) rstd gamma + beta, z = act(u) (+ residual)."""
    y = np.asarray(y, F64)
    R = y.shape[0]
    u = (y - per_row(mean, R, N, G)) * per_row(rstd, R, N, G) * np.asarray(gamma, F64) + np.asarray(beta, F64)
    z = act_apply(u, act)
    return u, (z if residual is None else z + np.asarray(residual, F64))


def bwd(dz, y, z, mean, rstd, gamma, beta, N, G, act):
    """(du, s1[G,C], s2[G,C], dgamma, dbeta, dy).  The activation's derivative comes from z when z is given (dvae_bn_bwd:
    z > 0, 1 - z^2), otherwise from the sign of u (dvae_bn_bwd_from_y; ReLU or none)."""
    dz, y = np.asarray(dz, F64), np.asarray(y, F64)
    R = y.shape[0]
    cnt = count(R, N, G)
    ga, rs = np.asarray(gamma, F64), per_row(rstd, R, N, G)
    yh = (y - per_row(mean, R, N, G)) * rs
    if z is None:
        assert act in (ACT_NONE, ACT_RELU)
        z = act_apply(yh * ga + np.asarray(beta, F64), act)
    z = np.asarray(z, F64)
    d = (z > 0).astype(F64) if act == ACT_RELU else 1.0 - z * z if act == ACT_TANH else 1.0
    du = dz * d
    s1, s2 = group_sum(du, R, N, G), group_sum(du * yh, R, N, G)
    dy = ga * rs * (du - per_row(s1, R, N, G) / cnt - yh * per_row(s2, R, N, G) / cnt)
    return du, s1, s2, s2.sum(0), s1.sum(0), dy


# ------------------------------------------------------------------ the bounds
def stats_bounds(y, N, G, eps, rm=None, rv=None, momentum=0.1, from_partials=False):
    """Reference and bounds of dvae_bn_stats_fwd / _finalize from the data y (fp32 values, or the float64 data the host
    summed into partials).  Keys: mean, var, rstd, tol_mean, tol_rstd, kappa, and with rm / rv: rm, rv, tol_rm, tol_rv."""
    y = np.asarray(y, F64)
    R = y.shape[0]
    cnt, a, c = count(R, N, G), tree_adds(R, from_partials), var_roundings(R, from_partials)
    mean, var, rstd = stats(y, N, G, eps)
    e1, e2 = group_sum(np.abs(y), R, N, G) / cnt, group_sum(y * y, R, N, G) / cnt
    dmean = (a + 17) * EPS64 * e1
    dvar = c * EPS64 * e2
    d = dvar / (var + float(eps))
    with np.errstate(divide="ignore", invalid="ignore"):
        cancel = np.where(d < 1.0, 1.0 / np.sqrt(np.maximum(1.0 - d, 1e-300)) - 1.0, np.inf)
        kappa = np.where(var > 0, mean * mean / np.where(var > 0, var, 1.0), np.inf)
    out = {"mean": mean, "var": var, "rstd": rstd, "kappa": kappa, "tol_mean": EPS32 * np.abs(mean) + dmean + FLOOR,
           "tol_rstd": rstd * (EPS32 + 4 * EPS64 + cancel), "rstd_cancel_over_eps32": cancel / EPS32}
    if rm is not None:
        mom = float(momentum)
        unb = var * cnt / (cnt - 1.0) if cnt > 1 else var
        dunb = dvar * (cnt / (cnt - 1.0) if cnt > 1 else 1.0)
        for key, r, x, dx in (("rm", rm, mean, dmean), ("rv", rv, unb, dunb)):
            r, tol = np.asarray(r, F64).copy(), 0.0
            for k in range(G):
                t1, t2 = (1.0 - mom) * r, mom * x[k]
                tol = abs(1.0 - mom) * tol * (1 + EPS32) + g(3) * (np.abs(t1) + np.abs(t2)) + abs(mom) * dx[k] + FLOOR
                r = t1 + t2
            out[key], out["tol_" + key] = r, tol
    return out


def tol_u(y, mean, rstd, gamma, beta, N, G):
    y = np.asarray(y, F64)
    R = y.shape[0]
    A = np.abs(y - per_row(mean, R, N, G)) * per_row(rstd, R, N, G) * np.abs(np.asarray(gamma, F64))
    return g(4) * (A + np.abs(np.asarray(beta, F64))) + FLOOR


def apply_bounds(y, mean, rstd, gamma, beta, residual, N, G, act):
    """Reference and bound of dvae_bn_apply_fwd from its inputs.  Keys: u, z, tol_u, tol_z."""
    u, z = apply(y, mean, rstd, gamma, beta, residual, N, G, act)
    tu = tol_u(y, mean, rstd, gamma, beta, N, G)
    if act == ACT_TANH:
        a = np.tanh(u)
        tz = tu / np.cosh(np.maximum(np.abs(u) - tu, 0.0)) ** 2 + TANHF_ROUNDINGS * EPS32 * np.abs(a) + FLOOR
    else:
        a, tz = act_apply(u, act), tu
    if residual is not None:
        tz = tz * (1 + EPS32) + EPS32 * (np.abs(a) + np.abs(np.asarray(residual, F64)))
    return {"u": u, "z": z, "tol_u": tu, "tol_z": tz}


def ambiguous_pairs(y, mean, rstd, gamma, beta, N, G):
    """[G, C] bool: the (group, channel) pairs holding an element whose float64 |u| lies within the forward bound of 0: the
    ReLU mask dvae_bn_bwd_from_y recomputes there is not determined by the inputs."""
    y = np.asarray(y, F64)
    R = y.shape[0]
    u, _ = apply(y, mean, rstd, gamma, beta, None, N, G, ACT_NONE)
    amb = np.abs(u) <= tol_u(y, mean, rstd, gamma, beta, N, G)
    return group_sum(amb, R, N, G) > 0


def bwd_bounds(dz, y, z, mean, rstd, gamma, beta, N, G, act, old_dgamma=None, old_dbeta=None, s12=None):
    """Reference and bounds of dvae_bn_bwd (z given) / dvae_bn_bwd_from_y (z None) from the launch's inputs.  s12: the
    device's own fp32 [G, C, 2] (s1, s2), which dy is judged with; without it dy is judged with the float64 sums and their
    bounds are carried.  Keys: s1, s2, dgamma, dbeta, dy and tol_ of each (dgamma / dbeta include old_*)."""
    dz, y = np.asarray(dz, F64), np.asarray(y, F64)
    R, C = y.shape
    cnt, b = count(R, N, G), tree_adds(R) + 16
    du, s1, s2, dgam, dbet, _ = bwd(dz, y, z, mean, rstd, gamma, beta, N, G, act)
    ga, rs = np.asarray(gamma, F64), per_row(rstd, R, N, G)
    yh = (y - per_row(mean, R, N, G)) * rs
    if act == ACT_TANH:
        zz = np.asarray(z, F64) ** 2
        ddu = EPS32 * np.abs(dz) * (zz + np.abs(1.0 - zz)) + EPS32 * np.abs(du)
    else:
        ddu = np.zeros_like(du)
    e1 = group_sum(ddu, R, N, G) + b * EPS64 * group_sum(np.abs(du), R, N, G)
    e2 = group_sum(np.abs(yh) * ddu + g(2) * np.abs(du * yh), R, N, G) + b * EPS64 * group_sum(np.abs(du * yh), R, N, G)
    out = {"s1": s1, "s2": s2, "tol_s1": e1 + EPS32 * np.abs(s1) + FLOOR, "tol_s2": e2 + EPS32 * np.abs(s2) + FLOOR}
    for key, tot, e, old in (("dgamma", dgam, e2, old_dgamma), ("dbeta", dbet, e1, old_dbeta)):
        old = np.zeros(C) if old is None else np.asarray(old, F64)
        out[key] = old + tot
        out["tol_" + key] = (e.sum(0) + EPS32 * np.abs(tot)) * (1 + EPS32) + EPS32 * np.abs(old + tot) + FLOOR
    if s12 is None:
        S1, S2, carry = s1, s2, (per_row(out["tol_s1"], R, N, G) + np.abs(yh) * per_row(out["tol_s2"], R, N, G)) / cnt
    else:
        S1, S2, carry = np.asarray(s12, F64)[..., 0], np.asarray(s12, F64)[..., 1], 0.0
    a1, a2 = per_row(S1, R, N, G) / cnt, yh * per_row(S2, R, N, G) / cnt
    out["dy"] = ga * rs * (du - a1 - a2)
    out["tol_dy"] = np.abs(ga * rs) * (g(8) * (np.abs(du) + np.abs(a1) + np.abs(a2)) + ddu + carry) + FLOOR
    return out


# Where the bound is +inf nothing is held (ratio 0): the families that share this module's bounds (elem_ref, audio_ref) mark
# the elements a kernel is not held at that way.
worst_ratio = functools.partial(ref_common.worst_ratio, inf_tol_unheld=True)


# ------------------------------------------------------------------ inputs of the tests (CPU and GPU alike)
# R, N, G, C and what the shape reaches in csrc/bn.hip
CASES = [
    (1, 1, 1, 4),            # cnt == 1, one quad, one row lane
    (2, 2, 2, 4),            # cnt == 1 per group
    (35, 5, 1, 80),          # partial chunk, C < 256
    (126, 6, 2, 260),        # second column of workgroups with one live quad
    (198, 66, 2, 512),       # more segments than rows per chunk, groups split inside a chunk
    (12400, 2, 2, 8),        # 194 chunks: unrolled finalize loop for some threads only
    (16400, 2, 2, 8),        # 257 chunks: unrolled loop, then tail
    (4112, 16, 2, 512),      # total4 = 526 336 > 2048 * 256: the grid-stride loops wrap for the last 2 048 quads only
]
# Seeds for which no (group, channel) pair of the case is ambiguous for the recomputed ReLU mask (asserted on the CPU in
# tests/test_bn_ref.py, on the device's own mean / rstd in tests/test_hip_bn.py, where at most 0.5 % may be).
SEEDS = {case: 100 + i for i, case in enumerate(CASES)}


def make_inputs(R, N, G, C, seed):
    """fp32 inputs of one case: y [R, C] with a mean in [-3, 3] and a standard deviation in [0.05, 2] of its own per channel,
    the second group shifted against the first by +-[0.5, 1.5]; gamma in +-[0.05, 1.5], every 16th channel (from 3) near
    +-1e-3; beta in +-0.3; dz and the residual uniform in +-1; old dgamma / dbeta uniform in +-2."""
    rs = np.random.RandomState(seed)
    mu, sd = rs.uniform(-3, 3, C), rs.uniform(0.05, 2, C)
    shift = rs.uniform(0.5, 1.5, C) * rs.choice([-1.0, 1.0], C)
    y = mu + shift * groups(R, N, G)[:, None] + sd * np.sqrt(3.0) * rs.uniform(-1, 1, (R, C))
    gamma = rs.uniform(0.05, 1.5, C) * rs.choice([-1.0, 1.0], C)
    gamma[3::16] = 1e-3 * rs.uniform(0.8, 1.2, len(gamma[3::16])) * rs.choice([-1.0, 1.0], len(gamma[3::16]))
    d = {"y": y, "gamma": gamma, "beta": rs.uniform(-0.3, 0.3, C), "dz": rs.uniform(-1, 1, (R, C)),
         "res": rs.uniform(-1, 1, (R, C)), "dgamma0": rs.uniform(-2, 2, C), "dbeta0": rs.uniform(-2, 2, C),
         "rm0": rs.uniform(-1, 1, C), "rv0": rs.uniform(0.5, 1.5, C)}
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in d.items()}


def cancellation_inputs(R=4096):
    """[R, 8] fp32: standard deviation 1e-2 around 0, 1, 1e1 ... 1e5, and one constant channel at 1e4."""
    rs = np.random.RandomState(7)
    off = np.array([0.0, 1.0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e4])
    y = off + 1e-2 * rs.standard_normal((R, 8))
    y[:, 7] = 1e4
    return np.ascontiguousarray(y, dtype=np.float32)


def exact_zero_case():
    """R = 64 rows of one group, C = 8: mean 0.5, rstd 2, gamma +-1, beta +-0: y = 0.5 (u = +-0) on a third of the elements, the
    next float above / below on the others (u = +-2^-23, -+2^-24 by the sign of gamma); dz in multiples of 1/64.  Every
    operation of the kernels is exact on this data, with or without contraction, so everything is compared exactly."""
    R, C = 64, 8
    rs = np.random.RandomState(31)
    k = (np.arange(R)[:, None] + np.arange(C)) % 3
    half = np.float32(0.5)
    y = np.where(k == 0, half, np.where(k == 1, np.nextafter(half, np.float32(1)), np.nextafter(half, np.float32(0)))).astype(np.float32)
    gamma = np.where(np.arange(C) % 2 == 0, 1.0, -1.0).astype(np.float32)
    beta = np.where(np.arange(C) % 4 < 2, 0.0, -0.0).astype(np.float32)
    dz = (rs.randint(-64, 65, (R, C)) / 64.0).astype(np.float32)
    return R, C, y, gamma, beta, dz


# ------------------------------------------------------------------ the kernels' statements in numpy float32
def _rows32(s, R, N, G):
    return np.asarray(s, F)[groups(R, N, G)]


def running_f32(r, xs, momentum, fma):
    """r' = (1 - mom) r + mom (float)x per group, fp32."""
    r, mom = np.asarray(r, F).copy(), F(momentum)
    for x in xs:
        xf = np.asarray(x, F64).astype(F)
        r = _fma(mom, xf, (F(1) - mom) * r) if fma else (F(1) - mom) * r + mom * xf
    return r


def apply_f32(y, mean, rstd, gamma, beta, residual, N, G, act, fma):
    """bn_apply_kernel, one rounding per operation; `fma`: the last product fused with the sum.  tanh: the float64 value
    rounded to fp32 (half a rounding: inside any TANHF_ROUNDINGS >= 0.5)."""
    y, ga, be = np.asarray(y, F), np.asarray(gamma, F), np.asarray(beta, F)
    R = y.shape[0]
    t = (y - _rows32(mean, R, N, G)) * _rows32(rstd, R, N, G)
    u = _fma(t, ga, be) if fma else t * ga + be
    z = np.maximum(u, F(0)) if act == ACT_RELU else np.tanh(u.astype(F64)).astype(F) if act == ACT_TANH else u
    return z if residual is None else z + np.asarray(residual, F)


def bwd_f32(dz, y, z, mean, rstd, gamma, beta, N, G, act, old_dgamma, old_dbeta, fma):
    """bn_partial_kernel<1> + bn_bwd_finalize_kernel + bn_bwd_apply_kernel: fp32 terms, float64 sums, fp32 s12.
    Returns (s12 [G, C, 2] fp32, dgamma, dbeta, dy)."""
    dz, y, ga = np.asarray(dz, F), np.asarray(y, F), np.asarray(gamma, F)
    R = y.shape[0]
    rs = _rows32(rstd, R, N, G)
    yh = (y - _rows32(mean, R, N, G)) * rs
    if z is None:
        u = _fma(yh, ga, np.asarray(beta, F)) if fma else yh * ga + np.asarray(beta, F)
        z = np.maximum(u, F(0)) if act == ACT_RELU else u
    z = np.asarray(z, F)
    if act == ACT_RELU:
        d = (z > 0).astype(F)
    elif act == ACT_TANH:
        d = _fma(-z, z, F(1)) if fma else F(1) - z * z
    else:
        d = F(1)
    du = dz * d
    s1, s2 = group_sum(du, R, N, G), group_sum(du.astype(F64) * yh.astype(F64), R, N, G)
    s12 = np.stack([s1, s2], -1).astype(F)
    dgamma = np.asarray(old_dgamma, F) + s2.sum(0).astype(F)
    dbeta = np.asarray(old_dbeta, F) + s1.sum(0).astype(F)
    inv = F(1) / (F(R // N) * F(N // G))
    S1, S2 = _rows32(s12[..., 0], R, N, G), _rows32(s12[..., 1], R, N, G)
    if fma:
        br = _fma(-(yh * S2), inv, _fma(-S1, inv, du))
    else:
        br = du - S1 * inv - yh * S2 * inv
    return s12, dgamma, dbeta, ga * rs * br
