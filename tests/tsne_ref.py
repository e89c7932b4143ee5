"""Float64 numpy restatement of the latent map (dvae_amd.latent_map, csrc/tsne.hip): the nearest
neighbour search, the perplexity search, the dense joint probabilities, the eight sums of a row, scikit-learn's update rule,
the whole embedding and the 1-NN speaker agreement; the bounds the four kernels are held to; fp32 walks in the kernels' own
column order; the planted cases.  Not a test module: tests/test_tsne_ref.py and tests/test_hip_tsne.py use it.

The bounds (EPS32 = 2^-24 is one rounding, g(k) = k EPS32 / (1 - k EPS32) is k of them compounded; K = ceil(N / 4) + 3 is
the number of additions a column's term can pass through: its wave's quarter and the three merges):

distance    d = sum_d (x_id - x_jd)^2 with dz = x_id - x_jd (one rounding, two on its square) and acc = fma(dz, dz, acc): a
            term passes through at most D roundings of the accumulator.  Every term is >= 0: |d~ - d| <= g(D + 2) d.
d'          max(d - d2min, 0) is 1-Lipschitz in d and rounds once: bdp = bd + EPS32 d'.
exponent    t = -beta d' (affinities: one product) or fma(-beta, d', -lnz) (forces): beta bdp + EPS32 |t|; the exponential
            is v_exp_f32 of t log2(e): the argument's conversion costs 2 |t| EPS32 and the instruction 1 ulp = 2 EPS32
            (the accounting of tests/latents_ref.py).  With tau their sum, e~ lies within exp(t +- tau) of e = exp(t).
            A flushed denormal is below 2^-126: FLOOR per column.
sums        one rounding per column of a quarter plus the merges: g(K) on the sum of the absolute terms.
affinities  lnz = logf(S0) (1 ulp), H = fma(beta, S1 / S0, lnz): the perturbations dS0, dS1 of the sums carried through the
            logarithm and the quotient (a division within 1 ulp), one rounding for the fma.
forces      p = (e_i + e_j) fp32(1 / 2N): three more roundings.  q = fma(dy1, dy1, dy0 dy0): g(4) relative; 1 + q one more;
            w = v_rcp_f32 (1 ulp): g(8) on w, g(17) on w w.  A: (p w) dy into an fma: g(10 + K) on the exact part.  R: w w
            dy: g(18 + K).  Z: g(8 + K).  p ln p: logf within 1 ulp and d(p ln p) / dp = 1 + ln p.  p ln w = -p log1pf(q):
            log1p(q) moves relatively no more than q does, log1pf within 1 ulp: g(7 + K).
update      Z and the KL sums in float64 (negligible, bounded by their own count of roundings); g = 4 fma(ex, A, -(R izf)),
            izf = fp32(1 / Z): two roundings on R / Z, one on the fma; the gains are exact in fp32 when upd g is not within
            the bound of zero (the generator keeps it ten bounds away); upd = fma(mom, upd, -(lr (gains g))): two roundings
            on the product, one on the fma; y += upd one more.
"""
import math

import numpy as np

from ref_common import EPS32, EPS64, F, F64, FLOOR, fma, g  # noqa: F401

MAX_D = 64                 # DVAE_LATENT_MAX_D
ENTROPY_TOL = 1e-5         # scikit-learn's _binary_search_perplexity
BETA_MAX = 2.0 ** 100
MIN_GAIN = 0.01
MAX_STEPS = 64


def K_of(N):
    return (N + 3) // 4 + 3


def quarters(N):
    q = (N + 3) // 4
    return [(w * q, min((w + 1) * q, N)) for w in range(4) if w * q < N]


# --------------------------------------------------------------------------------------------------------- distances
def dist2(x):
    """[N, N] float64 squared distances in the difference form"""
    x = np.asarray(x, F64)
    out = np.zeros((len(x), len(x)), F64)
    for d in range(x.shape[1]):
        dz = x[:, None, d] - x[None, :, d]
        out += dz * dz
    return out


def dist2_f32(x):
    """the kernels' own arithmetic: dz = x_i - x_j, acc = fma(dz, dz, acc), d ascending"""
    x = np.asarray(x, F)
    acc = np.zeros((len(x), len(x)), F)
    for d in range(x.shape[1]):
        dz = x[:, None, d] - x[None, :, d]
        acc = fma(dz, dz, acc)
    return acc


def dist_bound(d2, D):
    return g(D + 2) * d2 + FLOOR


def admissible(N, group=None):
    if group is None:
        return ~np.eye(N, dtype=bool)
    group = np.asarray(group)
    return group[:, None] != group[None, :]


def nearest(d2, group=None):
    """-> (d2min [N] (+inf without an admissible neighbour), arg [N] (-1 then)); ties go to the lowest index"""
    m = np.where(admissible(len(d2), group), d2, np.inf)
    arg = m.argmin(axis=1)
    best = m[np.arange(len(d2)), arg]
    return best, np.where(np.isfinite(best), arg, -1)


def nearest_margin(d2, D, group=None):
    """the smallest of (d_j - d_min) - bound(d_j) - bound(d_min) over the admissible j that are not exact ties of the
    minimum: positive when no rounding of the distances can change the arg-min"""
    m = np.where(admissible(len(d2), group), d2, np.inf)
    best = m.min(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        margin = np.where(np.isfinite(m) & (m > best), m - best - dist_bound(m, D) - dist_bound(best, D), np.inf)
    return float(margin.min())


# -------------------------------------------------------------------------------------------------- perplexity search
def entropy_at(d2, d2min, beta):
    """float64 (lnz, H) of every row at its beta, shifted by d2min"""
    dp = np.maximum(d2 - d2min[:, None], 0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-beta[:, None] * dp)
    np.fill_diagonal(e, 0.0)
    s0, s1 = e.sum(1), (dp * e).sum(1)
    lnz = np.log(s0)
    return lnz, lnz + beta * s1 / s0


def affinities(d2, perplexity, max_steps=MAX_STEPS, d2min=None):
    """van der Maaten's search for every row -> dict(beta, lnz, entropy, steps [N], d2min)"""
    N = len(d2)
    d2min = nearest(d2)[0] if d2min is None else np.asarray(d2min, F64)
    target = math.log(perplexity)
    b, lo, hi = np.ones(N), np.full(N, -np.inf), np.full(N, np.inf)
    steps, done = np.full(N, -1, np.int64), np.zeros(N, bool)
    lnz, H = np.zeros(N), np.zeros(N)
    for it in range(max_steps):
        l_, h_ = entropy_at(d2, d2min, b)
        lnz, H = np.where(done, lnz, l_), np.where(done, H, h_)
        diff = H - target
        conv = ~done & (np.abs(diff) <= ENTROPY_TOL)
        steps[conv] = it + 1
        done |= conv
        if done.all() or it + 1 == max_steps:
            break
        up, dn = ~done & (diff > 0), ~done & ~(diff > 0)
        lo = np.where(up, b, lo)
        hi = np.where(dn, b, hi)
        nb = np.where(up, np.where(np.isinf(hi), np.minimum(b * 2.0, BETA_MAX), (b + hi) * 0.5),
                      np.where(np.isinf(lo), b * 0.5, (b + lo) * 0.5))
        b = np.where(done, b, nb)
    return dict(beta=b, lnz=lnz, entropy=H, steps=steps, d2min=d2min)


def _exp_terms(t, tau):
    """e = exp(t) and the largest |e~ - e| for an exponent within tau of t"""
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp(t)
        return e, np.exp(np.minimum(t + tau, 700.0)) - e


def affinities_bound(d2, D, d2min, beta):
    """bounds of the device's lnz and entropy against entropy_at on the same (fp32) d2min and beta -> (blnz, bH)"""
    N, K = len(d2), K_of(len(d2))
    dp = np.maximum(d2 - d2min[:, None], 0.0)
    bdp = dist_bound(d2, D) + EPS32 * dp
    t = -beta[:, None] * dp
    tau = (beta[:, None] * bdp + EPS32 * np.abs(t) + (2.0 * np.abs(t) + 2.0) * EPS32) * (1.0 + EPS32)
    e, eE = _exp_terms(t, tau)
    off = ~np.eye(N, dtype=bool)
    e, eE = e * off, eE * off
    dS0 = (eE * (1.0 + g(K)) + e * g(K) + FLOOR).sum(1)
    dS1 = ((dp + bdp) * (e + eE) * (1.0 + g(K + 1)) - dp * e + FLOOR * (dp + 1.0)).sum(1)
    S0, S1 = e.sum(1), (dp * e).sum(1)
    lnz = np.log(S0)
    rel = dS0 / S0
    with np.errstate(divide="ignore", invalid="ignore"):
        blnz = np.where(rel < 1.0, -np.log1p(-np.minimum(rel, 1.0)), np.inf)      # not resolved: nothing is held
    blnz = blnz + 2.0 * EPS32 * (np.abs(lnz) + blnz) + FLOOR
    q = S1 / S0
    with np.errstate(divide="ignore", invalid="ignore"):
        bq = np.where(rel < 1.0, (dS1 + q * dS0) / np.maximum(S0 - dS0, FLOOR), np.inf)
    bq = bq + 2.0 * EPS32 * (q + bq)
    H = lnz + beta * q
    bH = blnz + beta * bq
    return blnz, bH + EPS32 * (np.abs(H) + bH) + FLOOR


def affinity_sums_f32(d32, d2min, beta):
    """fp32 (lnz, H) in dvae_tsne_affinities' order from its fp32 distances: per quarter the columns ascending, the quarters
    in wave order.  exp and ln are float64's, rounded once."""
    N = len(d32)
    d2min, beta = np.asarray(d2min, F), np.asarray(beta, F)
    rows = np.arange(N)
    tot0, tot1 = None, None
    for c0, c1 in quarters(N):
        s0, s1 = np.zeros(N, F), np.zeros(N, F)
        for j in range(c0, c1):
            dp = np.maximum(d32[:, j] - d2min, F(0))
            with np.errstate(under="ignore"):
                e = np.exp((-beta * dp).astype(F).astype(F64)).astype(F)
            e = np.where(rows != j, e, F(0))
            s0 = s0 + e
            s1 = fma(dp, e, s1)
        tot0, tot1 = (s0, s1) if tot0 is None else (tot0 + s0, tot1 + s1)
    lnz = np.log(tot0.astype(F64)).astype(F)
    return lnz, fma(beta, tot1 / tot0, lnz)


# --------------------------------------------------------------------------------------------------------- the forces
def conditional(d2, beta, d2min, lnz):
    """p_{j|i} [N, N] float64, zero on the diagonal"""
    with np.errstate(under="ignore"):
        c = np.exp(-beta[:, None] * np.maximum(d2 - d2min[:, None], 0.0) - lnz[:, None])
    np.fill_diagonal(c, 0.0)
    return c


def dense_P(d2, beta, d2min, lnz):
    c = conditional(d2, beta, d2min, lnz)
    return (c + c.T) / (2.0 * len(d2))


def row_sums(P, y, want_kl=True):
    """the eight sums of every row in float64 -> [N, 8]"""
    y = np.asarray(y, F64)
    dy = y[:, None, :] - y[None, :, :]
    q = dy[..., 1] * dy[..., 1] + dy[..., 0] * dy[..., 0]
    w = 1.0 / (1.0 + q)
    off = ~np.eye(len(y), dtype=bool)
    out = np.zeros((len(y), 8), F64)
    out[:, 0:2] = ((P * w)[..., None] * dy).sum(1)
    out[:, 2:4] = ((w * w)[..., None] * dy).sum(1)
    out[:, 4] = (w * off).sum(1)
    if want_kl:
        with np.errstate(divide="ignore", invalid="ignore"):
            out[:, 5] = np.where(P > 0, P * np.log(P), 0.0).sum(1)
        out[:, 6] = (-P * np.log1p(q)).sum(1)
        out[:, 7] = P.sum(1)
    return out


def kl_of(rows):
    """the KL from the row sums, float64 in row order"""
    r = np.asarray(rows, F64)
    Z = r[:, 4].sum()
    return float(r[:, 5].sum() - r[:, 6].sum() + math.log(Z) * r[:, 7].sum())


def gradient_of(rows, ex=1.0):
    r = np.asarray(rows, F64)
    return 4.0 * (ex * r[:, 0:2] - r[:, 2:4] / r[:, 4].sum())


def forces_bound(d2, D, beta, d2min, lnz, y):
    """bounds of dvae_tsne_forces' eight sums against row_sums(dense_P(...), y) -> [N, 8]"""
    N, K = len(d2), K_of(len(d2))
    y = np.asarray(y, F64)
    bd = dist_bound(d2, D)

    def side(b, dm, lz):      # the row's own term; the column's is its transpose
        dp = np.maximum(d2 - dm[:, None], 0.0)
        t = -b[:, None] * dp - lz[:, None]
        tau = (b[:, None] * (bd + EPS32 * dp) + EPS32 * np.abs(t) + (2.0 * np.abs(t) + 2.0) * EPS32) * (1.0 + EPS32)
        return _exp_terms(t, tau)

    e, eE = side(beta, d2min, lnz)
    off = ~np.eye(N, dtype=bool)
    e, eE = e * off, eE * off
    inv = 1.0 / (2.0 * N)
    p = (e + e.T) * inv
    bp = ((eE + eE.T) * (1.0 + g(3)) + (e + e.T) * g(3)) * inv + FLOOR
    dy = y[:, None, :] - y[None, :, :]
    q = dy[..., 1] * dy[..., 1] + dy[..., 0] * dy[..., 0]
    w = 1.0 / (1.0 + q)
    ady = np.abs(dy)
    out = np.zeros((N, 8), F64)
    out[:, 0:2] = ((w * (bp * (1.0 + g(10 + K)) + p * g(10 + K)))[..., None] * ady).sum(1)
    out[:, 2:4] = ((w * w * g(18 + K))[..., None] * ady).sum(1)
    out[:, 4] = (w * off * g(8 + K)).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        alp = np.where(p > 0, np.abs(np.log(p)), 0.0)
    out[:, 5] = (bp * (2.0 + alp) * (1.0 + g(3 + K)) + p * alp * g(3 + K) + 200.0 * FLOOR).sum(1)
    l1p = np.log1p(q)
    out[:, 6] = (l1p * (bp * (1.0 + g(7 + K)) + p * g(7 + K))).sum(1)
    out[:, 7] = (bp * (1.0 + g(K)) + p * g(K)).sum(1)
    return out + FLOOR


def forces_f32(d32, beta, d2min, lnz, y, want_kl=True):
    """dvae_tsne_forces' arithmetic in fp32 numpy, in its order -> [N, 8] fp32.  exp, ln, log1p and the reciprocal are
    float64's, rounded once."""
    N = len(d32)
    beta, d2min, lnz, y = (np.asarray(v, F) for v in (beta, d2min, lnz, y))
    inv2n = F(0.5 / N)
    rows = np.arange(N)
    total = None
    for c0, c1 in quarters(N):
        s = [np.zeros(N, F) for _ in range(8)]
        for j in range(c0, c1):
            d = d32[:, j]
            with np.errstate(under="ignore"):
                ei = np.exp(fma(-beta, np.maximum(d - d2min, F(0)), -lnz).astype(F64)).astype(F)
                ej = np.exp(fma(-beta[j], np.maximum(d - d2min[j], F(0)), -lnz[j]).astype(F64)).astype(F)
            on = rows != j
            p = np.where(on, (ei + ej) * inv2n, F(0)).astype(F)
            dy0, dy1 = y[:, 0] - y[j, 0], y[:, 1] - y[j, 1]
            q = fma(dy1, dy1, dy0 * dy0)
            wq = (1.0 / (F(1) + q).astype(F64)).astype(F)
            pw, w2 = p * wq, wq * wq
            s[0], s[1] = fma(pw, dy0, s[0]), fma(pw, dy1, s[1])
            s[2], s[3] = fma(w2, dy0, s[2]), fma(w2, dy1, s[3])
            s[4] = s[4] + np.where(on, wq, F(0))
            if want_kl:
                with np.errstate(divide="ignore", invalid="ignore"):
                    lp = np.where(p > 0, np.log(p.astype(F64)), 0.0).astype(F)
                s[5] = fma(p, lp, s[5])
                s[6] = fma(p, -np.log1p(q.astype(F64)).astype(F), s[6])
                s[7] = s[7] + p
        total = s if total is None else [a + b for a, b in zip(total, s)]
    return np.stack(total, axis=1)


# --------------------------------------------------------------------------------------------------------- the update
def update(rows, y, upd, gains, lr, momentum, ex):
    """scikit-learn's _gradient_descent step in float64 on the rows as given (the gains in fp32: they are exact there)
    -> dict(y, upd, gains, g, Z, kl)"""
    rows, y, upd = np.asarray(rows, F64), np.asarray(y, F64), np.asarray(upd, F64)
    grad = gradient_of(rows, ex)
    gn = np.where(upd * grad < 0.0, np.asarray(gains, F) + F(0.2), np.asarray(gains, F) * F(0.8)).astype(F)
    gn = np.maximum(gn, F(MIN_GAIN))
    un = momentum * upd - lr * (gn.astype(F64) * grad)
    return dict(y=y + un, upd=un, gains=gn, g=grad, Z=float(rows[:, 4].sum()), kl=kl_of(rows))


def update_bound(rows, y, upd, gains_new, lr, momentum, ex):
    """bounds of dvae_tsne_update against update() on the same fp32 inputs -> dict(g, upd, y, kl)"""
    rows, y, upd = np.asarray(rows, F64), np.asarray(y, F64), np.asarray(upd, F64)
    N = len(rows)
    Z = rows[:, 4].sum()
    rz = np.abs(rows[:, 2:4]) / Z
    grad = gradient_of(rows, ex)
    bg = 4.0 * (rz * (g(2) + N * EPS64) + EPS32 * np.abs(grad) / 4.0) * (1.0 + EPS32) + FLOOR
    gn = np.asarray(gains_new, F64)
    un = momentum * upd - lr * (gn * grad)
    bu = lr * gn * (bg + g(2) * (np.abs(grad) + bg)) + EPS32 * (np.abs(un) + lr * gn * bg) + FLOOR
    by = bu + EPS32 * (np.abs(y + un) + bu) + FLOOR
    k64 = (N + 16) * EPS64
    sums = np.abs(rows[:, 5]).sum() + np.abs(rows[:, 6]).sum() + (abs(math.log(Z)) + 1.0) * np.abs(rows[:, 7]).sum()
    return dict(g=bg, upd=bu, y=by, kl=4.0 * k64 * sums + FLOOR)


def embed(P, y0, iters, exaggeration_iters, exaggeration, lr, kl_every=50):
    """the whole descent in float64 on a dense P -> dict(y, kl (of the final y), trace [(iteration, kl before its update)])"""
    y = np.asarray(y0, F64).copy()
    upd, gains = np.zeros_like(y), np.ones(y.shape, F)
    trace = []
    for it in range(iters):
        early = it < exaggeration_iters
        want = it % kl_every == 0
        rows = row_sums(P, y, want_kl=want)
        if want:
            trace.append((it, kl_of(rows)))
        r = update(rows, y, upd, gains, lr, 0.5 if early else 0.8, exaggeration if early else 1.0)
        y, upd, gains = r["y"], r["upd"], r["gains"]
    return dict(y=y, kl=kl_of(row_sums(P, y)), trace=trace)


def pca_init(x, seed=0):
    """the first two principal components from the float64 D x D covariance, the first scaled to a standard deviation of
    1e-4; each component's sign makes its largest entry positive"""
    x = np.asarray(x, F64)
    xc = x - x.mean(0)
    N, D = x.shape
    if D < 2:
        y = np.concatenate([xc, np.random.default_rng(seed).standard_normal((N, 1))], axis=1)
    else:
        _, vec = np.linalg.eigh(xc.T @ xc / max(N - 1, 1))
        v = vec[:, ::-1][:, :2]
        v = v * np.where(v[np.abs(v).argmax(0), np.arange(2)] < 0, -1.0, 1.0)
        y = xc @ v
    sd = y[:, 0].std()
    return y / (sd if sd > 0 else 1.0) * 1e-4


def nn_agreement(arg, speakers):
    """the share of the rows with a neighbour whose neighbour has their speaker, and the count of the rows without one"""
    arg, speakers = np.asarray(arg), np.asarray(speakers)
    has = arg >= 0
    if not has.any():
        return float("nan"), int((~has).sum())
    return float(np.mean(speakers[arg[has]] == speakers[has])), int((~has).sum())


def chance(speakers):
    _, n = np.unique(np.asarray(speakers), return_counts=True)
    p = n / n.sum()
    return float((p * p).sum())


# --------------------------------------------------------------------------------------------------- the planted cases
def planted_speakers(seed=0, n_spk=4, per=64, D=4, spread=0.3, utt=8):
    """n_spk speakers x per points: centres 3 N(0, 1), spread 0.3, utterances of 8 chunks as the groups"""
    r = np.random.default_rng(seed)
    centres = 3.0 * r.standard_normal((n_spk, D))
    spk = np.repeat(np.arange(n_spk), per)
    x = centres[spk] + spread * r.standard_normal((n_spk * per, D))
    return dict(x=x.astype(F), speakers=spk.astype(np.int32), groups=(np.arange(n_spk * per) // utt).astype(np.int32))


def planted_independent(seed=0, n_spk=4, per=64, D=28, utt=8):
    """the same labels on a block that knows nothing of them"""
    r = np.random.default_rng(seed)
    spk = np.repeat(np.arange(n_spk), per)
    return dict(x=r.standard_normal((n_spk * per, D)).astype(F), speakers=spk.astype(np.int32),
                groups=(np.arange(n_spk * per) // utt).astype(np.int32))


# ------------------------------------------------------------------------------------- the shapes of the kernel tests
NS = [8, 63, 64, 65, 255, 256, 257, 1000]
SHAPES = [(1, 1), (2, 2), (4, 4), (5, 7), (28, 28), (32, 33), (64, 64)]      # (D, ld)
GROUP_OF = 4               # the groups of the kernel tests: four consecutive rows
_CASES = {}


def perplexity_of(N):
    return 2.0 if N == 8 else 5.0


def kernel_case(N, D, ld):
    """x [N, D] fp32 normal, with the planted rows: row 0 lies 300 and row 1 1e4 typical distances (sqrt(2 D)) from
    everything, in two directions; rows 2 and 3 are exact duplicates; row 4 lies close to them (its nearest neighbour is the
    tie {2, 3}); rows 5 and 6 are moved towards the two far rows so that these have a nearest neighbour no rounding can
    change.  y [N, 2] fp32 normal with rows 4 and 5 coincident.  The margins are asserted.  Cached: the float64 tables are
    computed once and shared; nobody writes into them."""
    key = (N, D, ld)
    if key in _CASES:
        return _CASES[key]
    rs = np.random.RandomState(1009 * D + N)
    x = rs.randn(N, D)
    u0 = np.where(np.arange(D) % 2, -1.0, 1.0) / math.sqrt(D)
    u1 = np.ones(D) / math.sqrt(D)
    typical = math.sqrt(2.0 * D)
    x[0] = 300.0 * typical * u0
    x[1] = 1e4 * typical * u1
    x[3] = x[2]
    x[4] = x[2] + 0.2 * N ** (-1.0 / D) * (0.5 + rs.rand(D))      # a fifth of the typical spacing of N points in D dimensions
    x[5] += 8.0 * u0
    x[6] += 8.0 * u1 * (1.5 if D == 1 else 1.0)
    x = x.astype(F)
    x[3] = x[2]
    group = (np.arange(N) // GROUP_OF).astype(np.int32)
    d2 = dist2(x)
    for grp in (None, group):
        m = nearest_margin(d2, D, grp)
        assert m > 0.0, (key, grp is not None, m)
    y = rs.randn(N, 2).astype(F)
    y[5] = y[4]
    full = np.full((N, ld), np.nan, F)
    full[:, :D] = x
    aff = affinities(d2, perplexity_of(N))
    c = dict(N=N, D=D, ld=ld, x=x, full=full, group=group, d2=d2, y=y, aff=aff, perplexity=perplexity_of(N))
    _CASES[key] = c
    return c


def forces_inputs(c):
    """the fp32 tables dvae_tsne_forces is given in the tests: the float64 search's, rounded"""
    a = c["aff"]
    return {k: a[k].astype(F) for k in ("beta", "d2min", "lnz")}


def update_case(c, ex=12.0):
    """rows [N, 8] fp32 (the float64 sums, rounded, then entries of A doubled until no upd g lies within ten bounds of zero),
    upd, gains fp32 -> dict"""
    t = {k: v.astype(F64) for k, v in forces_inputs(c).items()}
    rows = row_sums(dense_P(c["d2"], t["beta"], t["d2min"], t["lnz"]), c["y"]).astype(F)
    rs = np.random.RandomState(c["N"] + 7 * c["D"])
    upd = (rs.choice([-1.0, 1.0], (c["N"], 2)) * rs.uniform(0.5, 2.0, (c["N"], 2))).astype(F)
    upd[::5] = 0.0
    gains = rs.uniform(0.005, 3.0, (c["N"], 2)).astype(F)
    lr, mom = 200.0, 0.5
    for _ in range(40):
        r = update(rows, c["y"], upd, gains, lr, mom, ex)
        b = update_bound(rows, c["y"], upd, r["gains"], lr, mom, ex)
        bad = (upd != 0) & (np.abs(r["g"]) <= 10.0 * b["g"])
        if not bad.any():
            break
        rows[:, 0:2] = np.where(bad, np.where(rows[:, 0:2] == 0, F(1e-3), rows[:, 0:2] * F(2)), rows[:, 0:2])
    assert not bad.any()
    return dict(rows=rows, upd=upd, gains=gains, lr=lr, momentum=mom, ex=ex, ref=r, bound=b)
