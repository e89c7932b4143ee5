"""The float64 restatement of the modulation-spectrum and global-variance loss of the train step (ops.SmoothingPenaltyFn,
csrc/msloss.hip) and the bounds a launch is held to.  Not a test module: tests/test_msloss_ref.py checks
the restatement on the CPU, tests/test_hip_msloss.py and tests/test_hip_msloss_train.py hold the kernels and the step to it.
numpy only; the statements are the issue's, the bounds are derived here from u = 2^-53, 2^-24 and operation counts; neither
follows what some code computes.

Inputs: y [N, C, T] fp32 (N = 2 Bh, the x1 half first), its target x = (x1 | x2), a window D (even, 8 .. 128, T % D == 0; the
W = T / D windows of a row are disjoint, no taper), a floor f > 0; eps_ms = D f^2, eps_gv = f^2 (a white ripple of standard
deviation f has E|Y_k|^2 = D f^2 and variance f^2).
    per (row, window, bin): d_t = y_t - mean_t(y), Y_k = sum_t d_t e^{-2 pi i k t / D} for k = 1 .. H = D/2, the twiddles from the
      float64 table twiddle(D) read at k t mod D;  P_k = |Y_k|^2, s_k = ln(P_k + eps_ms), Delta = s - s^x
      L_ms = the mean of Delta^2 over all M = N W C H elements (nats^2)
    per (row, bin): m = the mean over the row's T frames, v = (1 / T) sum_t (y_t - m)^2, g = ln(v + eps_gv)
      L_gv = the mean of (g - g^x)^2 over N C
    penalty = w_ms L_ms + w_gv L_gv;  stats = (L_ms, L_gv, msd_db = (10 / ln 10) sqrt(L_ms), gv_ratio_db = (10 / ln 10) mean(g - g^x),
      penalty)
    dL_ms/dd_t = (4 / M) sum_k Delta_k / (P_k + eps_ms) (Re Y_k cos th_kt - Im Y_k sin th_kt), th_kt = 2 pi k t / D
    dL_ms/dy_t = that minus its mean over the window;  dL_gv/dy_t = (1 / (N C)) 2 (g - g^x) / (v + eps_gv) (2 / T) (y_t - m)
    dy = gscale (w_ms dL_ms + w_gv dL_gv), rounded once to fp32
With eps -> 0 the four figures are what section 4.14 defines per window and per utterance.

Bounds.  The device works in float64 on fp32 inputs and rounds once at a store, so a bound is 2^-24 |reference| plus what float64
roundings can add, carried through the formulas to first order with every denominator taken at its worst (x - e for x):
    em  = gamma(n / 16 + 6) sum|y| / n                      a mean of n frames: n / 16 additions a lane, four tree levels, one division
    eY  = gamma(D + 8) (sum|d_t| + D em)                    D products with twiddles good to 2 u, D additions, the centring
    eP  = 2 |Y| eY + eY^2 + 3 u P,   es = (eP + u (P + eps)) / (P + eps - eP) + 2 u |s|,   eD = es + es^x + u |Delta|
    L_ms: (sum (2 |Delta| eD + eD^2) + gamma(W H + nwg + 32) sum Delta^2) / M       nwg = N ceil(C / 16) partial sums
    ev  = gamma(T / 16 + 10) v + em^2,   eg = (ev + u (v + eps)) / (v + eps - ev) + 2 u |g|,   edg = eg + eg^x + u |dg|
    L_gv: (sum (2 |dg| edg + edg^2) + gamma(nwg + 48) sum dg^2) / (N C),   gv_ratio_db likewise from edg
    q = Delta / (P + eps):  eq = (eD + |q| eP) / (P + eps - eP) + 2 u |q|
    G_t = sum_k q_k (Re cos - Im sin):  eG = 1.5 sum_k (eq (|Y| + eY) + |q| eY) + gamma(2 H + 8) A,  A = 1.5 sum_k |q_k| |Y_k| >= |G_t|
    G_t - mean(G):  2 eG + 2 gamma(D / 16 + 12) A
    c = 2 dg / (v + eps):  ec = (2 edg + |c| ev) / (v + eps - ev) + 3 u |c|;   c (y_t - m):  ec (|y_t - m| + em) + |c| em + 2 u |c (y_t - m)|
    dy: gscale (a_ms e_ms + a_gv e_gv) + 8 u (the two terms' absolute values)
each float64 part taken TWICE (once for the device, once for this restatement, whose matrix products add in another order).  The
stabiliser keeps every denominator above eps, so every element is held: none is left out.
"""
import math

import numpy as np

from ref_common import EPS32, EPS64, FLOOR as FLOOR32

F32, F64 = np.float32, np.float64
U = EPS64
DB = 10.0 / math.log(10.0)
D_MIN, D_MAX = 8, 128            # DVAE_MODSPEC_DMIN / DMAX
FLOOR = 0.003                    # the default floor: 0.3 dB of the normalised 100 dB range (a setting, not a measured optimum)
BINS = 16                        # bins of a row per workgroup
WEIGHTS = (0.75, 0.5)            # w_ms, w_gv of the kernel suite
# (Bh, C, T, D) of the kernel suite: the tile remainder, D below 16 lanes a bin, several windows a row, the x1 | x2 boundary
SHAPES = [(1, 1, 8, 8), (1, 3, 24, 8), (3, 80, 64, 64), (2, 17, 128, 64), (1, 80, 256, 128)]
MUTATIONS = ("k0", "no_centring", "im_sign", "var_div_D", "sum_for_mean", "eps_without_D", "halves_swapped")


def gamma(n):
    return n * U / (1.0 - n * U)


def twiddle(D):
    return np.asarray([[math.cos(2.0 * math.pi * j / D), math.sin(2.0 * math.pi * j / D)] for j in range(D)], F64)


def default_window(T):
    return min(64, int(T))


def check_window(T, D):
    if D % 2 or not D_MIN <= D <= D_MAX or T % D:
        raise ValueError(f"a window of D={D} frames on T={T}: D even, in [{D_MIN}, {D_MAX}], T % D == 0")


def basis(D, k0=False):
    """cos, sin [K, D] of th_kt, k = 1 .. D/2 (k0: from 0), read from the table at k t mod D"""
    tw = twiddle(D)
    k = np.arange(0 if k0 else 1, D // 2 + 1)
    idx = (k[:, None] * np.arange(D)[None, :]) % D
    return tw[idx, 0], tw[idx, 1]


def kernel_case(Bh, C, T, D, seed=0):
    """seeded trajectories in [0, 1]: the target, a reconstruction that is a smoothed target plus a ripple, one constant bin"""
    rs = np.random.RandomState(1000 * Bh + 10 * C + T + D + seed)
    x = rs.uniform(0.0, 1.0, (2 * Bh, C, T))
    sm = (np.roll(x, 1, -1) + x + np.roll(x, -1, -1)) / 3.0
    y = np.clip(0.7 * sm + 0.3 * rs.uniform(0.0, 1.0, x.shape), 0.0, 1.0)
    y[0, C - 1, :] = 0.25
    x = x.astype(F32)
    return dict(y=y.astype(F32), x1=x[:Bh].copy(), x2=x[Bh:].copy())


def _side(a, D, floor, mut):
    """one trajectory [N, C, T] -> its window and row figures, float64"""
    a = np.asarray(a).astype(F64)
    N, C, T = a.shape
    W = T // D
    w = a.reshape(N, C, W, D)
    mean = w.sum(-1) / D
    d = w - (0.0 if mut == "no_centring" else mean[..., None])
    cs, sn = basis(D, k0=mut == "k0")
    re, im = d @ cs.T, -(d @ sn.T)
    if mut == "im_sign":
        im = -im
    eps_ms = (1.0 if mut == "eps_without_D" else D) * floor * floor
    P = re * re + im * im
    m = a.sum(-1) / T
    # (a shift of d leaves Y_k, k >= 1, where it is up to roundings: "no centring" is told apart by the variance)
    v = ((a - (0.0 if mut == "no_centring" else m[..., None])) ** 2).sum(-1) / (D if mut == "var_div_D" else T)
    eps_gv = floor * floor
    return dict(w=w, mean=mean, d=d, re=re, im=im, P=P, s=np.log(P + eps_ms), m=m, v=v, g=np.log(v + eps_gv), eps_ms=eps_ms,
                eps_gv=eps_gv, cs=cs, sn=sn)


def evaluate(y, x1, x2, D, floor=FLOOR, w_ms=WEIGHTS[0], w_gv=WEIGHTS[1], gscale=1.0, mut=None):
    """-> dict(stats [5], dy [N, C, T], and the intermediate figures the bounds are made of), float64"""
    y = np.asarray(y)
    N, C, T = y.shape
    check_window(T, D)
    if not floor > 0:
        raise ValueError("floor > 0")
    x = np.concatenate([x2, x1] if mut == "halves_swapped" else [x1, x2], 0)
    a, b = _side(y, D, floor, mut), _side(x, D, floor, mut)
    W, K = T // D, a["s"].shape[-1]
    M = N * W * C * K
    delta = a["s"] - b["s"]
    dg = a["g"] - b["g"]
    l_ms = (delta ** 2).sum() if mut == "sum_for_mean" else (delta ** 2).sum() / M
    l_gv = (dg ** 2).sum() / (N * C)
    pen = w_ms * l_ms + w_gv * l_gv
    stats = np.asarray([l_ms, l_gv, DB * math.sqrt(l_ms), DB * dg.sum() / (N * C), pen], F64)
    q = delta / (a["P"] + a["eps_ms"])
    G = (q * a["re"]) @ a["cs"] - (q * a["im"]) @ a["sn"]              # [N, C, W, D]; ("im_sign" leaves P alone and turns this)
    Gc = G - G.sum(-1, keepdims=True) / D
    c = 2.0 * dg / (a["v"] + a["eps_gv"])
    dev = np.asarray(y).astype(F64) - a["m"][..., None]
    t_ms = (w_ms * 4.0 / M) * Gc.reshape(N, C, T)
    t_gv = (w_gv * 2.0 / ((D if mut == "var_div_D" else T) * N * C)) * (c[..., None] * dev)
    return dict(stats=stats, dy=gscale * (t_ms + t_gv), a=a, b=b, delta=delta, dg=dg, q=q, c=c, dev=dev, t_ms=t_ms, t_gv=t_gv,
                M=M, gscale=gscale, w=(w_ms, w_gv))


def loss(y, x1, x2, D, floor=FLOOR, w_ms=WEIGHTS[0], w_gv=WEIGHTS[1]):
    return float(evaluate(y, x1, x2, D, floor, w_ms, w_gv)["stats"][4])


# ------------------------------------------------------------------------------------------------------------- the bounds
def _mean_err(absum, n):
    return gamma(n / 16.0 + 6) * absum / n


def _side_err(sd, D, T):
    """float64 error of one side's s and g, and of what they are made of"""
    em_w = _mean_err(np.abs(sd["w"]).sum(-1), D)
    eY = gamma(D + 8) * (np.abs(sd["d"]).sum(-1) + D * em_w)[..., None]
    Y = np.sqrt(sd["P"])
    P, eps = sd["P"], sd["eps_ms"]
    eP = 2.0 * Y * eY + eY * eY + 3.0 * U * P
    es = (eP + U * (P + eps)) / (P + eps - eP) + 2.0 * U * np.abs(sd["s"])
    em = _mean_err(np.abs(sd["w"]).sum((-1, -2)), T)
    v, eg_ = sd["v"], sd["eps_gv"]
    ev = gamma(T / 16.0 + 10) * v + em * em
    eg = (ev + U * (v + eg_)) / (v + eg_ - ev) + 2.0 * U * np.abs(sd["g"])
    return dict(eY=eY, Y=Y, eP=eP, es=es, em=em, ev=ev, eg=eg)


def bounds(r):
    """r = evaluate(...) -> (stats_bound [5], dy_bound [N, C, T])"""
    a, b, delta, dg = r["a"], r["b"], r["delta"], r["dg"]
    N, C, W, D = a["w"].shape
    T, H = W * D, D // 2
    nwg = N * -(-C // BINS)
    ea, eb = _side_err(a, D, T), _side_err(b, D, T)
    eD = ea["es"] + eb["es"] + U * np.abs(delta)
    edg = ea["eg"] + eb["eg"] + U * np.abs(dg)
    l_ms, l_gv = r["stats"][0], r["stats"][1]
    e_lms = 2.0 * ((2.0 * np.abs(delta) * eD + eD * eD).sum() + gamma(W * H + nwg + 32) * (delta ** 2).sum()) / r["M"]
    e_lgv = 2.0 * ((2.0 * np.abs(dg) * edg + edg * edg).sum() + gamma(nwg + 48) * (dg ** 2).sum()) / (N * C)
    e_gvr = 2.0 * DB * (edg.sum() + gamma(nwg + 48) * np.abs(dg).sum()) / (N * C)
    e_msd = DB * e_lms / (math.sqrt(l_ms) + math.sqrt(max(l_ms - e_lms, 0.0))) if l_ms > 0 else DB * math.sqrt(e_lms)
    w_ms, w_gv = r["w"]
    e_pen = w_ms * e_lms + w_gv * e_lgv + 4.0 * U * (w_ms * l_ms + w_gv * l_gv)
    sb = np.asarray([e_lms, e_lgv, e_msd + 4.0 * U * abs(r["stats"][2]), e_gvr, e_pen], F64) + EPS32 * np.abs(r["stats"]) + FLOOR32
    # the gradient
    q, P, eps = r["q"], a["P"], a["eps_ms"]
    eq = (eD + np.abs(q) * ea["eP"]) / (P + eps - ea["eP"]) + 2.0 * U * np.abs(q)
    A = 1.5 * (np.abs(q) * ea["Y"]).sum(-1)
    eG = 1.5 * (eq * (ea["Y"] + ea["eY"]) + np.abs(q) * ea["eY"]).sum(-1) + gamma(2 * H + 8) * A
    e_ms = 2.0 * eG + 2.0 * gamma(D / 16.0 + 12) * A                                   # [N, C, W]
    e_ms = np.repeat(e_ms[..., None], D, -1).reshape(N, C, T)
    c, v, eg_ = r["c"], a["v"], a["eps_gv"]
    ec = (2.0 * edg + np.abs(c) * ea["ev"]) / (v + eg_ - ea["ev"]) + 3.0 * U * np.abs(c)
    adev = np.abs(r["dev"])
    e_gv = ec[..., None] * (adev + ea["em"][..., None]) + (np.abs(c) * ea["em"])[..., None] + 2.0 * U * np.abs(c)[..., None] * adev
    gs = abs(r["gscale"])
    a_ms, a_gv = w_ms * 4.0 / r["M"], w_gv * 2.0 / (T * N * C)
    db = 2.0 * (gs * (a_ms * e_ms + a_gv * e_gv) + 8.0 * U * gs * (np.abs(r["t_ms"]) + np.abs(r["t_gv"])))
    return sb, db + EPS32 * np.abs(r["dy"]) + FLOOR32
