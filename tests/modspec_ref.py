"""The float64 restatement of the over-smoothing instruments (dvae_amd/modspec.py, csrc/modspec.hip)
and the bounds a launch is held to.  Not a test module: tests/test_modspec_ref.py checks the restatement on the CPU,
tests/test_hip_modspec.py holds the kernels and the engine to it.  numpy only; the statements are the issue's, the bounds are
derived here from u = 2^-53, 2^-24 and operation counts; neither follows what some code computes.

Global variance of utterance u, bin c: m = mean, v = population variance (divisor L) of the L frames, two passes.  The device
adds ceil(L / 64) frames per lane and then six tree levels: n = ceil(L / 64) + 6 additions on any path.  The restatement works in
long double, so its own error is its cast to float64:
    |m' - m| <= gamma(n + 2) sum|x| / L,   |v' - v| <= gamma(n + 5) v + (m' - m)^2   (sum (x - m')^2 = sum (x - m)^2 + L (m' - m)^2).

Modulation spectrum of a window, bin c: d_t = y_t - mean(y), Y_k = sum_t d_t e^{-2 pi i k t / D} for k = 1 .. D/2, s_k = ln max(|Y_k|^2,
FLOOR).  A recursive float64 sum of D terms is off by at most gamma(D) sum|d_t cos| in the real and gamma(D) sum|d_t sin| in the
imaginary part, together at most gamma(D) sum|d_t| in |Y_k| (Minkowski), and ln|Y|^2 moves by twice the relative error:
    |s' - s| <= 2 gamma(D) sum|d_t| / |Y_k| + 2^-24 |s|      (the second term: the one rounding to fp32 at the store).
The worst case of the sum is D times its typical size; that room covers the roundings of the twiddles, the square, the
logarithm and this restatement's own FFT.  The suite's inputs keep |Y_k| >= 1e-6 sum|d_t| (asserted there), so the first term is
below 2.9e-8 and NO element is left out.  The squares: q = fp32(s32^2) of the stored s32, so against s^2
    |q' - s^2| <= (2 |s| + e) e + 2^-24 (|s| + e)^2,   e the bound of s.

Postfilter, per window, bin and k:  r = max(sigma_n, SIGMA_MIN) / max(sigma_g, SIGMA_MIN);  s' = (1 - alpha) s + alpha (r (s - mu_g) +
mu_n);  lg = clamp((s' - s) / 2, +- max_gain_db ln 10 / 20);  Y'_k = Y_k e^lg;  y'_t = mean + (1 / D) sum_k c_k Re(Y'_k e^{2 pi i k t / D}), c_k
= 2, c_{D/2} = 1.  With eY = gamma(D) sum|d_t| the error of Y_k and es = 2 eY / |Y_k| that of s:
    elg = alpha |r - 1| es / 2 + 8 u (|s| + r (|s| + |mu_g|) + |mu_n|)       (the clamp does not increase it)
    eY' = e^lg (eY + |Y_k| (expm1(elg) + 4 u))
    |y'' - y'| <= 2 [ (1 / D) sum_k c_k eY'_k + gamma(D/2 + 2) (1 / D) sum_k c_k |Y'_k| + gamma(D + 2) max|y| ] + 2^-24 |y'| + FLOOR32
(the bracket twice: once for the device, once for this restatement's FFTs).  alpha = 0: the input's bits.

Overlap-add of filtered windows (tests/convert_ref.py states its arithmetic): the weights w_j / den are positive and sum to one,
so the windows' own bounds pass through as their weighted mean, to which the overlap-add's bound is added; one covering window:
the window's bound alone; an utterance with L < D: the input's bits.  The clamp to [0, 1] is 1-Lipschitz.
"""
import math

import numpy as np

from ref_common import EPS32, EPS64, FLOOR as FLOOR32
import convert_ref as CR

F32, F64 = np.float32, np.float64
U = EPS64
FLOOR = 1e-30                    # DVAE_MODSPEC_FLOOR
SIGMA_MIN = 1e-6                 # DVAE_MODSPEC_SIGMA_MIN
D_MIN, D_MAX = 8, 128
DB = 10.0 / math.log(10.0)
MIN_RATIO = 1e-6                 # the suite's inputs keep |Y_k| >= MIN_RATIO sum|d_t|


def gamma(n):
    return n * U / (1.0 - n * U)


def twiddle(D):
    return np.asarray([[math.cos(2.0 * math.pi * j / D), math.sin(2.0 * math.pi * j / D)] for j in range(D)], F64)


def weights(D):
    """c_k for k = 1 .. D/2"""
    c = np.full(D // 2, 2.0)
    c[-1] = 1.0
    return c


def frequencies(D):
    return np.arange(1, D // 2 + 1) * 16000.0 / (256.0 * D)


# --------------------------------------------------------------------------------------------------------- global variance
def gv(x, utt):
    """x [C, ld] fp32 packed, utt [nutt, 4] -> dict(m, v [nutt, C] float64, tol_m, tol_v)"""
    x = np.asarray(x, F32)
    C = x.shape[0]
    m, v, tm, tv = (np.zeros((len(utt), C), F64) for _ in range(4))
    for u, (col0, L, _, _) in enumerate(utt):
        seg = x[:, col0:col0 + L].astype(np.longdouble)
        mm = seg.sum(1) / L
        vv = ((seg - mm[:, None]) ** 2).sum(1) / L
        n = -(-L // 64) + 6
        m[u], v[u] = mm.astype(F64), vv.astype(F64)
        tm[u] = gamma(n + 2) * np.abs(seg).sum(1).astype(F64) / L + FLOOR32
        tv[u] = gamma(n + 5) * v[u] + tm[u] ** 2 + FLOOR32
    return dict(m=m, v=v, tol_m=tm, tol_v=tv)


# ----------------------------------------------------------------------------------------------------- modulation spectrum
def analyse(windows):
    """windows [..., D] (fp32 as the device sees them; float64 is kept, for the CPU properties) -> (mean [...], d [..., D],
    Y [..., D/2] complex: k = 1 .. D/2), float64"""
    y = np.asarray(windows).astype(F64)
    mean = y.sum(-1) / y.shape[-1]
    d = y - mean[..., None]
    return mean, d, np.fft.rfft(d, axis=-1)[..., 1:]


def log_power(Y):
    return np.log(np.maximum(Y.real ** 2 + Y.imag ** 2, FLOOR))


def ratio(d, Y):
    """|Y_k| / sum|d_t| (inf for an all-zero window): the suite asserts >= MIN_RATIO"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs(Y) / np.abs(d).sum(-1)[..., None]


def modspec(windows):
    """-> dict(s [..., D/2] float64, tol_s, q = s^2, tol_q, ratio)"""
    _, d, Y = analyse(windows)
    D = d.shape[-1]
    s = log_power(Y)
    with np.errstate(divide="ignore", invalid="ignore"):
        es = 2.0 * gamma(D) * np.abs(d).sum(-1)[..., None] / np.abs(Y)
    tol_s = es + EPS32 * np.abs(s)
    tol_q = (2.0 * np.abs(s) + tol_s) * tol_s + EPS32 * (np.abs(s) + tol_s) ** 2
    return dict(s=s, tol_s=tol_s, q=s * s, tol_q=tol_q, ratio=ratio(d, Y))


def rows(windows):
    """windows [nwin, C, D] -> (rows [nwin C, D] float64: s | s^2, tol) in the layout of dvae_modspec_windows"""
    r = modspec(windows)
    n, C, H = r["s"].shape
    return (np.concatenate([r["s"], r["q"]], -1).reshape(n * C, 2 * H),
            np.concatenate([r["tol_s"], r["tol_q"]], -1).reshape(n * C, 2 * H))


def stored_rows(windows):
    """what the device stores when it rounds the restatement's s once: s32 | fp32(s32^2), as fp32 [nwin C, D]"""
    s = log_power(analyse(windows)[2])
    n, C, H = s.shape
    s32 = s.astype(F32)
    return np.concatenate([s32, (s32.astype(F64) ** 2).astype(F32)], -1).reshape(n * C, 2 * H)


def group_sum(rows32, order, first, C):
    """dvae_modspec_group_sum: rows32 [nwin C, D] fp32 -> sums [G, C, D]: sequential float64 sums in the order listed"""
    rows32 = np.asarray(rows32, F32)
    D = rows32.shape[1]
    r = rows32.reshape(-1, C, D).astype(F64)
    sums = np.zeros((len(first) - 1, C, D), F64)
    for g in range(len(first) - 1):
        for i in range(first[g], first[g + 1]):
            if 0 <= order[i] < r.shape[0]:
                sums[g] = sums[g] + r[order[i]]
    return sums


def mu_sigma(s_sum, s_sq, n):
    """the host arithmetic of ModSpecStats.mean / .std"""
    mu = s_sum / n
    return mu, np.maximum(np.sqrt(np.maximum(s_sq / n - mu * mu, 0.0)), SIGMA_MIN)


def window_stats(windows, rounded=True):
    """windows [n, C, D] of one group -> (mu, sigma [C, D/2]).  rounded: from s and s^2 as the device stores them (fp32);
    otherwise from the float64 s of the definition."""
    if rounded:
        r = stored_rows(windows).astype(F64)
        n, C, H = windows.shape[0], windows.shape[1], windows.shape[2] // 2
        r = r.reshape(n, C, 2 * H)
        s, q = r[..., :H], r[..., H:]
    else:
        s = log_power(analyse(windows)[2])
        q = s * s
    acc_s, acc_q = np.zeros(s.shape[1:], F64), np.zeros(s.shape[1:], F64)
    for w in range(s.shape[0]):
        acc_s, acc_q = acc_s + s[w], acc_q + q[w]
    return mu_sigma(acc_s, acc_q, s.shape[0])


def score(mu_a, lnv_a, mu_b, lnv_b):
    """mu [C, D/2], lnv [C] (the mean of ln v over the utterances) -> msd_db, gv_ratio_db, profile [D/2]"""
    diff = mu_a - mu_b
    return dict(msd_db=DB * math.sqrt(float(np.mean(diff * diff))), gv_ratio_db=DB * float(np.mean(lnv_a - lnv_b)),
                profile=diff.mean(0))


# ------------------------------------------------------------------------------------------------------------- postfilter
def max_log_gain(max_gain_db):
    return max_gain_db * math.log(10.0) / 20.0


def filter_windows(windows, mu_n, sigma_n, mu_g, sigma_g, alpha, max_gain_db=12.0, with_tol=True):
    """windows [nwin, C, D], statistics [C, D/2] -> (y' [nwin, C, D] float64, tol or None).  alpha = 0: the input (tol 0)."""
    windows = np.asarray(windows)
    if alpha == 0.0:
        return windows.astype(F64), (np.zeros(windows.shape, F64) if with_tol else None)
    mean, d, Y = analyse(windows)
    D = d.shape[-1]
    s = log_power(Y)
    r = np.maximum(sigma_n, SIGMA_MIN) / np.maximum(sigma_g, SIGMA_MIN)
    sp = (1.0 - alpha) * s + alpha * (r * (s - mu_g) + mu_n)
    cap = max_log_gain(max_gain_db)
    lg = np.clip(0.5 * (sp - s), -cap, cap)
    c = weights(D)
    Yp = Y * np.exp(lg)
    spec = np.concatenate([np.zeros(Yp.shape[:-1] + (1,), complex), Yp], -1)
    out = mean[..., None] + np.fft.irfft(spec, n=D, axis=-1)
    if not with_tol:
        return out, None
    absY = np.abs(Y)
    eY = gamma(D) * np.abs(d).sum(-1)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        es = np.where(absY > 0, 2.0 * eY / absY, 0.0)
    elg = 0.5 * alpha * np.abs(r - 1.0) * es + 8.0 * U * (np.abs(s) + r * (np.abs(s) + np.abs(mu_g)) + np.abs(mu_n))
    eYp = np.exp(lg) * (eY + absY * (np.expm1(elg) + 4.0 * U))
    f64 = ((c * eYp).sum(-1) / D + gamma(D // 2 + 2) * (c * np.abs(Yp)).sum(-1) / D
           + gamma(D + 2) * np.abs(windows.astype(F64)).max(-1))
    return out, 2.0 * f64[..., None] + EPS32 * np.abs(out) + FLOOR32


def cut(lengths, D, hop):
    """the plan of dvae_amd.modspec.plan: convert_ref.plan with batch 1; an utterance with L < D has no window (nwin = 0 in its
    row, its window of the list a padding window) -> utt, win (int64), ld, the number of real windows"""
    utt, win, ld, _ = CR.plan(lengths, D, hop, 1)
    for u in range(len(utt)):
        if utt[u][1] < D:
            win[utt[u][2]:utt[u][2] + utt[u][3], 0] = -1
            utt[u][3] = 0
    return utt, win, ld, int((win[:, 0] >= 0).sum())


def windows_of(packed, utt, win, D):
    """convert_ref.mel_to_windows in the dtype of `packed`"""
    out = np.zeros((len(win), packed.shape[0], D), packed.dtype)
    for w, (u, f0) in enumerate(win):
        if u >= 0:
            n = min(D, utt[u][1] - f0)
            out[w, :, :n] = packed[:, utt[u][0] + f0:utt[u][0] + f0 + n]
    return out


def overlap_add(y, tol, utt, win, w32, base):
    """y, tol [nwin, C, D] float64 (filtered windows and their bounds), base [C, ld] fp32: what the output buffer held ->
    (ref [C, ld] float64 clamped to [0, 1] where written, tol [C, ld], written [C, ld] bool)"""
    w = np.asarray(w32, F32).astype(F64)
    _, C, D = y.shape
    ref, tl = np.asarray(base).astype(F64).copy(), np.zeros(base.shape, F64)
    written = np.zeros(base.shape, bool)
    for col0, L, win0, nw in utt:
        if nw < 1:
            continue
        num, mag, et = np.zeros((C, L), F64), np.zeros((C, L), F64), np.zeros((C, L), F64)
        den, cnt = np.zeros(L, F64), np.zeros(L, np.int64)
        one, one_t = np.zeros((C, L), F64), np.zeros((C, L), F64)
        for k in range(win0, win0 + nw):
            f0 = win[k][1]
            num[:, f0:f0 + D] = num[:, f0:f0 + D] + w * y[k]
            mag[:, f0:f0 + D] = mag[:, f0:f0 + D] + w * np.abs(y[k])
            et[:, f0:f0 + D] = et[:, f0:f0 + D] + w * tol[k]
            den[f0:f0 + D] = den[f0:f0 + D] + w
            cnt[f0:f0 + D] += 1
            one[:, f0:f0 + D], one_t[:, f0:f0 + D] = y[k], tol[k]
        assert (cnt >= 1).all(), "a frame no window covers"
        many = cnt > 1
        r = np.where(many, num / den, one)
        t = np.where(many, et / den + EPS32 * np.abs(num / den) + 2.0 * (cnt + 2) * EPS64 * mag / den + FLOOR32, one_t)
        ref[:, col0:col0 + L], tl[:, col0:col0 + L] = np.clip(r, 0.0, 1.0), t
        written[:, col0:col0 + L] = True
    return ref, tl, written


def postfilter(mels, D, hop, mu_n, sigma_n, mu_g, sigma_g, alpha, max_gain_db=12.0):
    """mels: list of [C, L] (fp32; float64 is kept) -> list of (ref [C, L] float64, tol [C, L]; tol 0: the input's bits).  The
    restatement of ModSpec.postfilter: pack, cut, filter, cross-fade with sin^2, clamp."""
    mels = [np.asarray(m) for m in mels]
    if alpha == 0.0:
        return [(m.astype(F64), np.zeros(m.shape, F64)) for m in mels]
    utt, win, ld, _ = cut([m.shape[1] for m in mels], D, hop)
    packed = np.zeros((mels[0].shape[0], ld), np.result_type(*[m.dtype for m in mels]))
    for m, (col0, L, _, _) in zip(mels, utt):
        packed[:, col0:col0 + L] = m
    y, tol = filter_windows(windows_of(packed, utt, win, D), mu_n, sigma_n, mu_g, sigma_g, alpha, max_gain_db)
    ref, tl, _ = overlap_add(y, tol, utt, win, CR.window(D).astype(F32), packed)
    return [(ref[:, col0:col0 + L], tl[:, col0:col0 + L]) for col0, L, _, _ in utt]


def group_stats(groups, D, hop):
    """{name: [mel [C, L] fp32, ...]} -> the fields of a ModSpecStats as ModSpec.stats fills them (the float64 s and s^2 of the
    definition summed window by window; v and ln max(v, FLOOR) utterance by utterance; an utterance with L < D nowhere), and
    under tol_<field> the sum of the addends' bounds: what the device's sums, of its fp32 rows, may differ by."""
    names = list(groups)
    C, H = np.asarray(groups[names[0]][0]).shape[0], D // 2
    out = dict(names=names, D=D, hop=hop, windows=np.zeros(len(names), np.int64), utterances=np.zeros(len(names), np.int64))
    for k, shape in (("s_sum", (C, H)), ("s_sq", (C, H)), ("v_sum", (C,)), ("lnv_sum", (C,))):
        out[k], out["tol_" + k] = np.zeros((len(names),) + shape, F64), np.zeros((len(names),) + shape, F64)
    for g, name in enumerate(names):
        for m in groups[name]:
            m = np.asarray(m, F32)
            if m.shape[1] < D:
                continue
            utt, win, _, _ = cut([m.shape[1]], D, hop)
            w = windows_of(m, utt, win, D)
            r, t = (a.reshape(-1, C, D) for a in rows(w))
            for i in range(len(r)):
                out["s_sum"][g], out["s_sq"][g] = out["s_sum"][g] + r[i, :, :H], out["s_sq"][g] + r[i, :, H:]
                out["tol_s_sum"][g] += t[i, :, :H]
                out["tol_s_sq"][g] += t[i, :, H:]
            out["windows"][g] += len(r)
            q = gv(m, [(0, m.shape[1], 0, 0)])
            v, tv = q["v"][0], q["tol_v"][0]
            out["v_sum"][g], out["lnv_sum"][g] = out["v_sum"][g] + v, out["lnv_sum"][g] + np.log(np.maximum(v, FLOOR))
            out["tol_v_sum"][g] += tv
            out["tol_lnv_sum"][g] += -np.log1p(-np.minimum(tv / np.maximum(v, FLOOR), 0.5)) + 4.0 * U * np.abs(np.log(np.maximum(v, FLOOR)))
            out["utterances"][g] += 1
    return out


# ------------------------------------------------------------------------------------------------------------ restoration
def attenuate(windows, a):
    """windows [..., D] float64 -> the same with modulation component k scaled by a[k - 1] (the mean kept), float64"""
    w = np.asarray(windows, F64)
    spec = np.fft.rfft(w, axis=-1)
    spec[..., 1:] = spec[..., 1:] * a
    return np.fft.irfft(spec, n=w.shape[-1], axis=-1)


def restoration_tol(natural, generated32, a, max_gain_db=12.0):
    """natural [n, C, D] fp32 windows, generated32 = fp32(attenuate(natural, a)): the bound within which the device's
    postfilter at alpha = 1, with statistics the device took from the two sets themselves, gives back `natural`.
    In exact arithmetic s_G = s_N + 2 ln a, sigma_G = sigma_N, the gain is 1 / a and the filter restores N.  What moves it:
      the rounding of the generated windows to fp32: |dG_k| <= sum_t |dd_t| <= 2 D 2^-24 max|g|, so s_G is off by
          delta = -2 ln(1 - |dG_k| / |G_k|) per window, and the window's mean by 2^-24 max|g|;
      the fp32 stores of s and s^2: e = 2^-24 |s| (+ delta and the float64 term for the generated set) per stored s, hence
          |dmu| <= max_w e,  |d(sigma^2)| <= max_w[(2 |s| + e) e + 2^-24 (|s| + e)^2] + 2 |mu| |dmu| + dmu^2,  |dsigma| <= |d(sigma^2)| / sigma;
      so |r - 1| <= (dsigma_N + dsigma_G) / (sigma - dsigma_G) and the log-gain is off by
          elg = (|r - 1| (|s_G - mu_G| + delta + dmu_G) + dmu_N + dmu_G) / 2;
      the restored coefficient by |G_k| / a (expm1(elg)) + |dG_k| e^elg / a;  the output adds the filter's own bound.
    -> tol [n, C, D]"""
    natural = np.asarray(natural, F32)
    g64 = np.asarray(generated32, F32).astype(F64)
    D = natural.shape[-1]
    assert (np.abs(np.log(a)) < max_log_gain(max_gain_db)).all(), "the attenuation must lie inside the gain clamp"
    _, _, N = analyse(natural)
    _, dG, G = analyse(generated32)
    sN, sG = log_power(N), log_power(G)
    dGk = 2.0 * D * EPS32 * np.abs(g64).max(-1)[..., None]
    x = dGk / np.abs(G)
    assert (x < 0.5).all()
    delta = -2.0 * np.log1p(-x)
    eN = modspec(natural)["tol_s"]
    eG = modspec(generated32)["tol_s"] + delta

    def moved(s, e):
        mu, sigma = mu_sigma(s.sum(0), (s * s).sum(0), s.shape[0])
        dmu = e.max(0)
        dvar = ((2.0 * np.abs(s) + e) * e + EPS32 * (np.abs(s) + e) ** 2).max(0) + 2.0 * np.abs(mu) * dmu + dmu * dmu
        return mu, sigma, dmu, dvar / sigma

    _, sig, dmuN, dsN = moved(sN, eN)
    muG, _, dmuG, dsG = moved(sG, eG)
    assert (sig > 2.0 * dsG).all(), "too few windows for a spread the roundings leave alone"
    r1 = (dsN + dsG) / (sig - dsG)
    elg = 0.5 * (r1 * (np.abs(sG - muG) + delta + dmuG) + dmuN + dmuG)
    eY = (np.abs(G) * np.expm1(elg) + dGk * np.exp(elg)) / a
    c = weights(D)
    own = filter_windows(generated32, *window_stats(natural), *window_stats(generated32), 1.0, max_gain_db)[1]
    return ((c * eY).sum(-1) / D + EPS32 * np.abs(g64).max(-1))[..., None] + own


# ----------------------------------------------------------------------------------------------------------------- inputs
def trajectories(rng, shape):
    """seeded random trajectories in [0, 1] along the last axis: a smoothed part (what a mel does) and a white part (so that
    every modulation frequency carries energy), fp32"""
    n = shape[-1]
    white = rng.rand(*shape)
    slow = rng.rand(*shape[:-1], n + 8)
    slow = np.stack([slow[..., j:j + n] for j in range(9)], 0).mean(0)
    return (0.6 * slow + 0.4 * white).astype(F32)


def case_lengths(D):
    return (D - 1, D, D + 1, 2 * D - 1, 3 * D + 5)
