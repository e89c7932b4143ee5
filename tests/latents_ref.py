"""Float64 numpy restatement of the latent report (dvae_amd.latents): the device tables, the
pairwise log-densities and their log-sum-exps, the report's quantities, the error bounds the two kernels are held to, and
an fp32 walk in dvae_latent_lse's own column order.  Not a test module: tests/test_latents_ref.py and
tests/test_hip_latents.py use it.  Shapes: mu / lv / eps / z / a / h [N, D]; an LSE table [rows, D + 3]: the D dimensions, then
style (d < S), content (d >= S), joint.

The bounds (EPS32 = 2^-24 is one rounding, g(k) = k EPS32 / (1 - k EPS32) is k of them compounded):

tables      expf is within 1 ulp = 2 EPS32 (the HIP math library's documented error).  z = fma(expf(lv / 2), eps, mu): the
            exponential's 2 roundings on the product, one on the sum; a = -(c32 + lv / 2), c32 the fp32 constant ln(2 pi) / 2:
            one rounding of the constant, one of the sum; h = expf(-lv) / 2: 2 roundings, the halving exact.
t           dz = z - mu, q = dz dz, t = fma(-h, q, a): three roundings on h dz^2, one on t:
            tau = g(3) h dz^2 + EPS32 |t|, scaled by (1 + EPS32) for the cross term.
block sums  k terms added one rounding each: tau_block = sum tau_d + g(k) sum |t_d|; joint = style + content adds one.
LSE, data   L is convex with gradient gamma (the softmax weights): a perturbation |delta_j| <= tau_j moves L down by at
            most B0 = sum gamma_j tau_j, and up by at most sum gamma_j tau_j exp(tau_j + B0) (along the way the weights
            grow by no more than that factor); L is also 1-Lipschitz in the largest |delta_j|.  The smaller of the two.
LSE, sums   term j of s = sum exp(t_j - M) passes through at most 1 + R + 3 exponentials (its own, the R rescales of its
            wave's quarter, three merges), whose arguments telescope to M - t_j; an argument x costs its own rounding and
            the rounding of x log2(e), |x| EPS32 each, and v_exp_f32 1 ulp: (2 |x| + 2) EPS32 per exponential.  Weighted by
            gamma, sum gamma_j (M - t_j) <= the entropy of gamma <= ln n.  The additions: one rounding per column of the
            quarter (n_w = ceil(n / 4)), two per merge.  Together K = 2 ln n + 2 (R + 4) + n_w + 6 roundings on s, so g(K)
            on ln s; logf is within 1 ulp of ln s <= ln n; the last addition rounds L.  R is counted on the data: column j
            of a quarter can rescale only if t_j + tau_j exceeds every earlier t_k - tau_k of the quarter.
            A flushed denormal exponential is below 2^-126 beside s >= 1: FLOOR per column.
"""
import math

import numpy as np

from ref_common import EPS32, EPS64, F, F64, FLOOR, fma, g  # noqa: F401

LOG_2PI = math.log(2.0 * math.pi)
HALF_LOG_2PI = 0.5 * LOG_2PI
ACTIVE_VAR = 0.01          # Burda et al.: a unit is active when the variance of its posterior mean exceeds this
MIN_SPEAKER_CHUNKS = 8
MAX_D = 64                 # DVAE_LATENT_MAX_D
CHUNK = 128                # rows per block of the [rows, cols, D] intermediates


# ------------------------------------------------------------------------------------------------------------ tables
def tables(mu, lv, eps, dtype=F):
    """float64 z, a, h from (mu, lv, eps), rounded once to `dtype` -> (z, mu, a, h)"""
    mu, lv, eps = (np.asarray(v, F64) for v in (mu, lv, eps))
    z = mu + np.exp(0.5 * lv) * eps
    a = -0.5 * (LOG_2PI + lv)
    h = 0.5 * np.exp(-lv)
    return z.astype(dtype), mu.astype(dtype), a.astype(dtype), h.astype(dtype)


def tables_bound(mu, lv, eps):
    """elementwise bounds of dvae_latent_tables' z, a, h against float64 on the fp32 inputs -> (bz, ba, bh)"""
    mu, lv, eps = (np.asarray(v, F64) for v in (mu, lv, eps))
    sd = np.exp(0.5 * lv)
    z = mu + sd * eps
    a = -0.5 * (LOG_2PI + lv)
    h = 0.5 * np.exp(-lv)
    bz = g(2) * sd * np.abs(eps) * (1 + EPS32) + EPS32 * np.abs(z) + FLOOR
    ba = (EPS32 * np.abs(a) + EPS32 * HALF_LOG_2PI) * (1 + 2 * EPS32) + FLOOR
    bh = g(2) * h + FLOOR
    return bz, ba, bh


# --------------------------------------------------------------------------------------------------- pairwise terms
def pair_terms(z, mu, a, h, S):
    """z [n, D] against columns mu, a, h [m, D] -> t [n, m, D + 3] float64: the D dimensions, style, content, joint"""
    z, mu, a, h = (np.asarray(v, F64) for v in (z, mu, a, h))
    t = a[None] - h[None] * (z[:, None, :] - mu[None]) ** 2
    st, ct = t[..., :S].sum(-1), t[..., S:].sum(-1)
    return np.concatenate([t, st[..., None], ct[..., None], (st + ct)[..., None]], axis=-1)


def pair_tau(z, mu, a, h, S, t):
    """the bound of the kernel's fp32 t, style, content and joint against `t` of pair_terms -> [n, m, D + 3]"""
    z, mu, a, h = (np.asarray(v, F64) for v in (z, mu, a, h))
    D = z.shape[1]
    hq = h[None] * (z[:, None, :] - mu[None]) ** 2
    td = t[..., :D]
    tau = (g(3) * hq + EPS32 * np.abs(td)) * (1 + EPS32)
    ab = np.abs(td)
    ts = tau[..., :S].sum(-1) + g(S) * ab[..., :S].sum(-1)
    tc = tau[..., S:].sum(-1) + g(D - S) * ab[..., S:].sum(-1)
    tj = ts + tc + EPS32 * (np.abs(t[..., D + 2]) + ts + tc)
    return np.concatenate([tau, ts[..., None], tc[..., None], tj[..., None]], axis=-1)


def lse64(t):
    """log-sum-exp over axis 1 of t [n, m, C] -> [n, C]"""
    m = t.max(axis=1)
    return m + np.log(np.exp(t - m[:, None]).sum(axis=1))


def quarters(ncols):
    """the column partition of dvae_latent_lse: wave w takes [w q, min((w + 1) q, ncols)), q = ceil(ncols / 4)"""
    q = (ncols + 3) // 4
    return [(w * q, min((w + 1) * q, ncols)) for w in range(4) if w * q < ncols]


def rescale_count(t, tau):
    """R of the module docstring: per (row, output) the largest number, over the quarters, of columns behind a quarter's
    first that could become its running maximum in fp32 -> [n, C]"""
    R = np.zeros((t.shape[0], t.shape[2]), np.int64)
    for c0, c1 in quarters(t.shape[1]):
        if c1 - c0 < 2:
            continue
        low = np.maximum.accumulate(t[:, c0:c1] - tau[:, c0:c1], axis=1)
        R = np.maximum(R, ((t[:, c0 + 1:c1] + tau[:, c0 + 1:c1]) > low[:, :-1]).sum(axis=1))
    return R


def lse_bound_from(t, tau, L):
    """the bound of the module docstring for every (row, output) -> [n, C]"""
    n = t.shape[1]
    with np.errstate(over="ignore", invalid="ignore"):
        gam = np.exp(t - L[:, None])
        b0 = (gam * tau).sum(axis=1)
        up = np.exp(t - L[:, None] + tau + b0[:, None]) * tau
        up = np.where(np.isfinite(up), up, np.inf).sum(axis=1)
    data = np.minimum(np.maximum(b0, up), tau.max(axis=1))
    K = 2.0 * math.log(n) + 2.0 * (rescale_count(t, tau) + 4) + (n + 3) // 4 + 6
    sums = g(K) + 2 * EPS32 * math.log(n) + EPS32 * (np.abs(L) + 1.0) + FLOOR * n
    return data + sums


def lse_tables(z, mu, a, h, S, rows, cols, bound=False):
    """rows = (row0, nrows), cols = (col0, ncols) -> L [nrows, D + 3] float64 on the tables as given (and its bound)"""
    (r0, nr), (c0, nc) = rows, cols
    L = np.empty((nr, z.shape[1] + 3), F64)
    B = np.empty_like(L) if bound else None
    cm, ca, ch = mu[c0:c0 + nc], a[c0:c0 + nc], h[c0:c0 + nc]
    for i in range(0, nr, CHUNK):
        zz = z[r0 + i:r0 + min(nr, i + CHUNK)]
        t = pair_terms(zz, cm, ca, ch, S)
        L[i:i + len(zz)] = lse64(t)
        if bound:
            B[i:i + len(zz)] = lse_bound_from(t, pair_tau(zz, cm, ca, ch, S, t), L[i:i + len(zz)])
    return (L, B) if bound else L


# ----------------------------------------------------------------------------------- the kernel's walk in fp32 (numpy)
def _update(m, s, t):
    hi, lo = np.maximum(m, t), np.minimum(m, t)
    with np.errstate(invalid="ignore"):
        e = np.exp((lo - hi).astype(F)).astype(F)
    s = np.where(t > m, fma(s, e, F(1)), (s + e).astype(F))
    return hi, s


def lse_f32(z, mu, a, h, S, rows, cols):
    """dvae_latent_lse's arithmetic in fp32 numpy, in its order: per quarter the columns ascending from (m, s) = (-inf, 0),
    the quarters merged in wave order, L = m + ln s.  exp and ln are numpy's.  -> [nrows, D + 3] fp32"""
    z, mu, a, h = (np.asarray(v, F) for v in (z, mu, a, h))
    (r0, nr), (c0, nc) = rows, cols
    D = z.shape[1]
    zz = z[r0:r0 + nr]
    acc = None
    for q0, q1 in quarters(nc):
        m, s = np.full((nr, D + 3), -np.inf, F), np.zeros((nr, D + 3), F)
        for j in range(c0 + q0, c0 + q1):
            dz = (zz - mu[j][None]).astype(F)
            t = fma(-h[j][None], (dz * dz).astype(F), a[j][None])
            st, ct = np.zeros(nr, F), np.zeros(nr, F)
            for d in range(D):
                if d < S:
                    st = (st + t[:, d]).astype(F)
                else:
                    ct = (ct + t[:, d]).astype(F)
            m, s = _update(m, s, np.concatenate([t, st[:, None], ct[:, None], (st + ct).astype(F)[:, None]], axis=1))
        if acc is None:
            acc = (m, s)
        else:
            m0, s0 = acc
            hi = np.maximum(m, m0)
            p = (s * np.exp((m - hi).astype(F)).astype(F)).astype(F)
            acc = (hi, fma(s0, np.exp((m0 - hi).astype(F)).astype(F), p))
    m, s = acc
    return (m + np.log(s).astype(F)).astype(F)


# ---------------------------------------------------------------------------------------------------------- the report
def entropy(counts):
    p = np.asarray(counts, F64) / np.sum(counts)
    p = p[p > 0]
    return float(-(p * np.log(p)).sum())


def speaker_jobs(speakers):
    """speakers [N] sorted labels -> [(first row, count)] per run of equal labels"""
    speakers = np.asarray(speakers)
    cut = np.flatnonzero(np.diff(speakers)) + 1
    first = np.concatenate([[0], cut])
    return list(zip(first.tolist(), np.diff(np.concatenate([first, [len(speakers)]])).tolist()))


def quantities(z, mu, a, h, S, speakers, L_all, L_own):
    """the report's figures from the tables (float64 arithmetic on them as given) and the LSE tables of the global job
    (L_all [N, D + 3]) and of the speakers' jobs (L_own [N, D + 3]) -> dict"""
    z, mu, a, h, L_all, L_own = (np.asarray(v, F64) for v in (z, mu, a, h, L_all, L_own))
    N, D = z.shape
    lnN = math.log(N)
    own_d = a - h * (z - mu) ** 2
    prior_d = -0.5 * LOG_2PI - 0.5 * z * z
    Ld = L_all[:, :D] - lnN
    out = {"n": N, "ln_n": lnN}
    for name, sl, col in (("style", slice(0, S), D), ("content", slice(S, D), D + 1), ("joint", slice(0, D), D + 2)):
        own, prior, marg, Lb = own_d[:, sl].sum(1), prior_d[:, sl].sum(1), Ld[:, sl].sum(1), L_all[:, col] - lnN
        out[name] = dict(mi=float(np.mean(own - Lb)), tc=float(np.mean(Lb - marg)), dwkl=float(np.mean(marg - prior)),
                         kl_sample=float(np.mean(own - prior)))
    out["shared"] = float(np.mean(L_all[:, D + 2] - L_all[:, D] - L_all[:, D + 1] + lnN))
    jobs = speaker_jobs(speakers)
    keep = np.zeros(N, bool)
    ln_ng = np.zeros(N, F64)
    for r0, n in jobs:
        keep[r0:r0 + n] = n >= MIN_SPEAKER_CHUNKS
        ln_ng[r0:r0 + n] = math.log(n)
    out["speaker_entropy"] = entropy([n for _, n in jobs])
    for name, col in (("style", D), ("content", D + 1)):
        v = (L_own[:, col] - ln_ng) - (L_all[:, col] - lnN)
        out["speaker_info_" + name] = float(np.mean(v[keep])) if keep.any() else float("nan")
    return out


def report(mu, lv, eps, speakers, S, dtype=F):
    """the whole report in float64 on the tables rounded to `dtype` -> dict (quantities + the tables and LSE tables)"""
    z, mu_t, a, h = (v.astype(F64) for v in tables(mu, lv, eps, dtype))
    N = len(z)
    L_all = lse_tables(z, mu_t, a, h, S, (0, N), (0, N))
    L_own = np.concatenate([lse_tables(z, mu_t, a, h, S, (r0, n), (r0, n)) for r0, n in speaker_jobs(speakers)])
    out = quantities(z, mu_t, a, h, S, speakers, L_all, L_own)
    out.update(tables=(z, mu_t, a, h), L_all=L_all, L_own=L_own)
    return out


def host_stats(mu, lv, S):
    """per dimension: analytic kl_d = mean (mu^2 + e^lv - lv - 1) / 2, var_i(mu_id), mean posterior variance, active"""
    mu, lv = np.asarray(mu, F64), np.asarray(lv, F64)
    kl = 0.5 * (mu * mu + np.exp(lv) - lv - 1.0).mean(0)
    var_mu = mu.var(0)
    return dict(kl=kl, var_mu=var_mu, mean_var=np.exp(lv).mean(0), active=var_mu > ACTIVE_VAR)


# --------------------------------------------------------------------------------------------------- the planted cases
def planted_gaussian(seed, independent=False, N=2048, rho=0.8):
    """mu ~ N(0, [[1, rho], [rho, 1]]) (independent: the second column redrawn), sigma = 0.5, D = 2, S = 1"""
    r = np.random.default_rng(seed)
    mu = r.standard_normal((N, 2)) @ np.linalg.cholesky(np.array([[1.0, rho], [rho, 1.0]])).T
    eps = r.standard_normal((N, 2))
    if independent:
        mu[:, 1] = r.standard_normal(N)
    lv = np.full((N, 2), 2.0 * math.log(0.5))
    return dict(mu=mu.astype(F), lv=lv.astype(F), eps=eps.astype(F), speakers=np.zeros(N, np.int32), S=1)


def planted_speakers(seed, per=256, sigma=0.5):
    """4 speakers x `per` chunks, S = 2, content 3: style means 10 (+-e1, +-e2) + 0.3 normal, content means normal"""
    r = np.random.default_rng(seed)
    centres = 10.0 * np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]])
    spk = np.repeat(np.arange(4), per)
    N = len(spk)
    mu = np.concatenate([centres[spk] + 0.3 * r.standard_normal((N, 2)), r.standard_normal((N, 3))], axis=1)
    lv = np.full((N, 5), 2.0 * math.log(sigma))
    eps = r.standard_normal((N, 5))
    return dict(mu=mu.astype(F), lv=lv.astype(F), eps=eps.astype(F), speakers=spk.astype(np.int32), S=2)


# ------------------------------------------------------------------------------------- the shapes of the kernel tests
NCOLS = [1, 2, 63, 64, 65, 255, 256, 257, 1000]
NROWS = [1, 64, 65, 130]
SHAPES = [(1, 0, 1), (1, 1, 1), (2, 1, 2), (5, 2, 7), (32, 4, 32), (64, 16, 64)]      # (D, S, ld)
ROW0, COL0 = 3, 5          # where the jobs of the kernel tests begin in their tables


def kernel_case(D, S, ld, ncols, nrows=130):
    """Tables [n, ld] (NaN outside the D columns) for a job of `nrows` rows from ROW0 against `ncols` columns from COL0.
    Column COL0 has lv = -20 and column COL0 + 1 lv = +10; row ROW0 lies 300 and row ROW0 + 1 1e4 of the largest posterior
    standard deviations beyond every mean.  A case with fewer rows is a prefix of the 130-row one.
    -> dict(z, mu, a, h [n, D] fp32, full = the four [n, ld] arrays)"""
    rs = np.random.RandomState(7919 * D + 31 * S + ncols)
    n = max(ROW0 + 130, COL0 + ncols) + 2
    mu = rs.randn(n, D)
    lv = rs.uniform(-3.0, 1.0, (n, D))
    lv[COL0] = -20.0
    if ncols > 1:
        lv[COL0 + 1] = 10.0
    eps = rs.randn(n, D)
    z, mu32, a, h = tables(mu, lv, eps)
    sd = float(np.exp(0.5 * lv[COL0:COL0 + ncols].max()))
    far = np.abs(mu).max() + sd
    z[ROW0] = (far * 300.0 * np.where(np.arange(D) % 2, -1.0, 1.0)).astype(F)
    z[ROW0 + 1] = F(far * 1e4)
    full = []
    for v in (z, mu32, a, h):
        f = np.full((n, ld), np.nan, F)
        f[:, :D] = v
        full.append(f)
    return dict(z=z, mu=mu32, a=a, h=h, full=full, n=n)
