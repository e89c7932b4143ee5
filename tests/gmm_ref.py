"""Float64 numpy restatement of the GMM-UBM speaker verification (dvae_amd.verify): the device
tables, the per-frame log-likelihood, the EM statistics and M-step, MAP adaptation, the likelihood ratio, the two error
bounds the kernels are held to, and an fp32 walk in the kernel's order.  Not a test module: tests/test_gmm_ref.py and
tests/test_hip_gmm.py use it.  Shapes: x [N, D], a [K], mu / prec [K, D], l / gamma / q [N, K].
"""
import math

import numpy as np

from ref_common import EPS32, EPS64, F, F64, FLOOR, fma  # noqa: F401

LOG_2PI = math.log(2.0 * math.pi)
VAR_FLOOR = 0.01        # of the global per-dimension variance
WEIGHT_FLOOR = 1e-6


def tables(w, mu, var, dtype=F):
    """(w, mu, var) float64 -> the device's model: a [K], mu [K, D], prec [K, D], computed in float64, rounded once
    (dtype=float64: not rounded, for the properties of EM itself)."""
    w, mu, var = np.asarray(w, F64), np.asarray(mu, F64), np.asarray(var, F64)
    a = np.log(w) - 0.5 * np.sum(LOG_2PI + np.log(var), axis=1)
    return a.astype(dtype), mu.astype(dtype), (1.0 / var).astype(dtype)


def loglik(x, a, mu, prec):
    """float64 on the tables as given -> l [N, K], lse [N], gamma [N, K], q [N, K] (q = 1/2 sum_d (x - mu)^2 prec)."""
    x, a, mu, prec = (np.asarray(v, F64) for v in (x, a, mu, prec))
    q = 0.5 * np.einsum("nkd,kd->nk", (x[:, None, :] - mu[None]) ** 2, prec)
    l = a[None] - q
    m = l.max(axis=1)
    lse = m + np.log(np.exp(l - m[:, None]).sum(axis=1))
    return l, lse, np.exp(l - lse[:, None]), q


def loglik_f32(x, a, mu, prec):
    """the kernel's own walk in fp32: q by one fma per dimension, d ascending; l = a - q / 2 (one rounding); the maximum;
    the sum of exp(l - max), k ascending; lse = max + ln(sum); gamma = exp(l - max) / sum.  -> l, lse, gamma (fp32).  exp
    and ln are numpy's."""
    x, a, mu, prec = (np.asarray(v, F) for v in (x, a, mu, prec))
    N, K, D = x.shape[0], a.shape[0], x.shape[1]
    q = np.zeros((N, K), F)
    for d in range(D):
        df = (x[:, d, None] - mu[None, :, d]).astype(F)
        q = fma((df * df).astype(F), prec[None, :, d], q)
    l = fma(F(-0.5), q, a[None])
    m = l.max(axis=1)
    e = np.exp((l - m[:, None]).astype(F)).astype(F)
    s = np.zeros(N, F)
    for k in range(K):
        s = (s + e[:, k]).astype(F)
    lse = (m + np.log(s).astype(F)).astype(F)
    return l, lse, (e / s[:, None]).astype(F)


def lse_bound(a, gamma, q, D):
    """|lse - lse64| <= (D + K + 16) 2^-24 (1 + sum_k gamma_kt (|a_k| + q_kt)), per frame"""
    a, gamma, q = np.asarray(a, F64), np.asarray(gamma, F64), np.asarray(q, F64)
    K = a.shape[0]
    return (D + K + 16) * EPS32 * (1.0 + np.sum(gamma * (np.abs(a)[None] + q), axis=1))


def gamma_bound(a, gamma, q, D):
    """|gamma - gamma64| <= gamma64 (b_kt + b_t) + 2^-23, b_t the lse bound, b_kt = (D + 16) 2^-24 (1 + |a_k| + q_kt)"""
    a, gamma, q = np.asarray(a, F64), np.asarray(gamma, F64), np.asarray(q, F64)
    b_kt = (D + 16) * EPS32 * (1.0 + np.abs(a)[None] + q)
    return gamma * (b_kt + lse_bound(a, gamma, q, D)[:, None]) + 2.0 ** -23


def stats(x, gamma):
    """n [K], f [K, D], s [K, D]: float64 sums of gamma, gamma x, gamma x^2"""
    x, gamma = np.asarray(x, F64), np.asarray(gamma, F64)
    return gamma.sum(axis=0), gamma.T @ x, gamma.T @ (x * x)


def stats_abs(x, gamma):
    """the same sums over |term|: what a float64 summation error is relative to"""
    x, gamma = np.abs(np.asarray(x, F64)), np.abs(np.asarray(gamma, F64))
    return gamma.sum(axis=0), gamma.T @ x, gamma.T @ (x * x)


def sum_bound(n_terms, abs_sum):
    """|float64 sum in any order - exact| <= (n + 2) 2^-53 sum |term|"""
    return (n_terms + 2) * EPS64 * np.asarray(abs_sum, F64)


def pack_stats(n, f, s, lse_sum):
    """the layout of dvae_gmm_estep's stats: per component {n_k, f_k [D], s_k [D]}, then sum_t lse_t"""
    return np.concatenate([np.concatenate([n[:, None], f, s], axis=1).reshape(-1), [lse_sum]])


def unpack_stats(v, K, D):
    v = np.asarray(v, F64)
    rec = v[:K * (1 + 2 * D)].reshape(K, 1 + 2 * D)
    return rec[:, 0].copy(), rec[:, 1:1 + D].copy(), rec[:, 1 + D:].copy(), float(v[-1])


def global_variance(x):
    x = np.asarray(x, F64)
    return (x * x).mean(axis=0) - x.mean(axis=0) ** 2


def m_step(n, f, s, N, mu_old, var_old, gvar):
    """w = n / N, mu = f / n, var = max(s / n - mu^2, 0.01 gvar); a component with n_k < D + 1 keeps its mean and
    variance; weights floored at 1e-6 and renormalised"""
    n, f, s = np.asarray(n, F64), np.asarray(f, F64), np.asarray(s, F64)
    D = f.shape[1]
    ok = n >= D + 1
    nn = np.where(ok, n, 1.0)[:, None]
    mu = np.where(ok[:, None], f / nn, mu_old)
    var = np.where(ok[:, None], np.maximum(s / nn - mu * mu, VAR_FLOOR * np.asarray(gvar, F64)[None]), var_old)
    w = np.maximum(n / N, WEIGHT_FLOOR)
    return w / w.sum(), mu, var


def em(x, w, mu, var, iters, gvar=None, dtype=F):
    """`iters` EM iterations from (w, mu, var) on the tables rounded to `dtype` -> (w, mu, var, [mean log-likelihood per
    frame])"""
    x = np.asarray(x, F64)
    gvar = global_variance(x) if gvar is None else gvar
    lls = []
    for _ in range(iters):
        _, lse, gamma, _ = loglik(x, *tables(w, mu, var, dtype))
        lls.append(float(lse.sum() / len(x)))
        w, mu, var = m_step(*stats(x, gamma), len(x), mu, var, gvar)
    return w, mu, var, lls


def map_adapt(w, mu, var, n, f, T, relevance=16.0):
    """MAP of weights and means, alpha_k = n_k / (n_k + r): mu' = alpha f / n + (1 - alpha) mu, w' proportional to
    alpha n / T + (1 - alpha) w, scaled to the total weight of w; variances kept"""
    w, mu, n, f = (np.asarray(v, F64) for v in (w, mu, n, f))
    with np.errstate(invalid="ignore", divide="ignore"):
        alpha = np.where(n > 0, n / (n + relevance), 0.0)
        mean = np.where(n[:, None] > 0, f / np.where(n > 0, n, 1.0)[:, None], mu)
    mu2 = alpha[:, None] * mean + (1.0 - alpha[:, None]) * mu
    w2 = alpha * n / T + (1.0 - alpha) * w
    return w2 * (w.sum() / w2.sum()), mu2, np.asarray(var, F64).copy()


def llr(x, model, ubm):
    """mean per-frame log-likelihood ratio of frames x: model and ubm are (w, mu, var)"""
    return float(np.mean(loglik(x, *tables(*model))[1] - loglik(x, *tables(*ubm))[1]))


def score_order_sum(lse, wg=256):
    """sum of fp32 lse values in dvae_gmm_score's order: thread i adds frames i, i + 256, ... (float64), then the xor tree
    over the 64 lanes of each wave (offsets 32 .. 1) and the four waves in order"""
    lse = np.asarray(lse, F).astype(F64)
    acc = np.zeros(wg, F64)
    for i in range(0, len(lse), wg):
        part = lse[i:i + wg]
        acc[:len(part)] = acc[:len(part)] + part
    lane = np.arange(64)
    waves = []
    for w0 in range(0, wg, 64):
        v = acc[w0:w0 + 64].copy()
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[lane ^ o]
        waves.append(v[0])
    return ((waves[0] + waves[1]) + waves[2]) + waves[3]


# --------------------------------------------------------------------------------------------- the planted two speakers
def planted_speakers(seed=0, D=5, centres=3, sigma=0.4, train=300, segments=12, seg_frames=50):
    """Two speakers, `centres` centres each at N(0, 1.5^2) + N(0, 1) (a shared draw plus the speaker's own), frames
    N(centre, sigma^2): -> dict(train [2][train, D], test [(speaker, [seg_frames, D])] * segments), fp32-representable"""
    rs = np.random.RandomState(seed)
    shared = rs.randn(centres, D) * 1.5
    cs = [shared + rs.randn(centres, D) for _ in range(2)]

    def draw(sp, n):
        return (cs[sp][rs.randint(0, centres, n)] + sigma * rs.randn(n, D)).astype(F).astype(F64)

    tr = [draw(0, train), draw(1, train)]
    te = [(i % 2, draw(i % 2, seg_frames)) for i in range(segments)]
    return dict(train=tr, test=te, D=D)


def init_from_frames(x, K, seed):
    """the trainer's start: K distinct frames drawn by default_rng(seed) as means, the global variance, uniform weights"""
    x = np.asarray(x, F64)
    idx = np.random.default_rng(seed).choice(len(x), size=K, replace=False)
    return np.full(K, 1.0 / K), x[idx].copy(), np.tile(global_variance(x), (K, 1)), idx


def m_step_bounds(n, f, s, dn, df, ds, N, gvar_floor_active=None):
    """|n' - n| <= dn, |f' - f| <= df, |s' - s| <= ds propagated through m_step (components with n well above D + 1):
    -> bounds on w (floored, renormalised), mu = f / n and var = max(s / n - mu^2, floor), each with a few float64
    roundings of slack.  mu' - mu = df / n' - mu dn / n'; the floor is 1-Lipschitz."""
    n, f, s = np.asarray(n, F64), np.asarray(f, F64), np.asarray(s, F64)
    lo = (n - dn)[:, None]
    mu = f / n[:, None]
    dmu = (df + np.abs(mu) * dn[:, None]) / lo
    dvar = (ds + (s / n[:, None]) * dn[:, None]) / lo + (2.0 * np.abs(mu) + dmu) * dmu
    w = np.maximum(n / N, WEIGHT_FLOOR)
    dw_raw = dn / N
    W, dW = w.sum(), dw_raw.sum()
    dw = (dw_raw + (w / W) * dW) / (W - dW)
    slack = lambda v: 1e-14 * (1.0 + np.abs(v))
    return dw + slack(w), dmu + slack(mu), dvar + slack(s / n[:, None])


def synthetic_voice(n, f0, formants, seed, sr=16000, bandwidth=180.0):
    """a harmonic series at f0 whose amplitudes follow a fixed formant envelope (a sum of Gaussians at `formants` Hz over a
    small floor), random phases, white noise 20 dB below: float32 [n]"""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / sr
    x = np.zeros(n)
    for k in range(1, int(0.45 * sr / f0) + 1):
        fk = k * f0
        amp = 0.02 + sum(np.exp(-0.5 * ((fk - fm) / bandwidth) ** 2) for fm in formants)
        x += amp * np.sin(2 * np.pi * fk * t + rs.uniform(0, 2 * np.pi))
    x = 0.1 * x / np.sqrt(np.mean(x ** 2))
    return (x + rs.randn(n) * 0.1 * 10 ** (-20 / 20)).astype(F)


VOICES = {"va": (500.0, 1500.0, 2500.0), "vb": (700.0, 1100.0, 3000.0)}      # two fixed formant envelopes


def voice_corpus(utts=6, seconds=1.0, sr=16000):
    """{voice: [waveform] * utts}: F0 varied over the same range for both voices, so that identity is in the envelope"""
    return {name: [synthetic_voice(int(sr * seconds), 100.0 + 9.0 * ((3 * i + j) % utts), fm, seed=10 * j + i)
                   for i in range(utts)] for j, (name, fm) in enumerate(sorted(VOICES.items()))}
