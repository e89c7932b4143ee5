"""The float64 restatement of the two validation kernels of csrc/val.hip and the rounding bounds one launch is held to.  Not
a test module: tests/test_val_ref.py proves the restatement against oracle.dvae_ref's loss (the reference's
loss_functionGVAE2, model/disentangled_vae.py:310-327, as its test() sums it, model/variational_base_vae.py:105-123),
tests/test_hip_val.py holds the kernels to it.  The formulas are the model's, the bounds are derived below; neither follows
what some code computes.

Notation of tests/elem_ref.py: eps32 = 2^-24 one fp32 rounding, eps64 = 2^-53, g(k) k roundings compounded, X =
EXPF_ROUNDINGS (the device's expf lies within X eps32 exp(x) of exp(x)), E = exp(lv) in float64, FLOOR = 2^-126.

pair_metrics, row b (the reference's terms with batch_size = 1)
    L1 columns 1..4: sum over the pair's n_per elements of |x - r|.  The difference rounds once in fp32 (exact when it is
    denormal: gradual underflow), |.| and the widening are exact, every addition is float64: a thread adds at most
    ceil(n_per / 256) + 3 terms (whole float4s), 6 butterfly steps over the lanes, 3 additions over the waves, 16 more for the
    reference's own pairwise sum:
        a1 = ceil(n_per / 256) + 28,      e_L1 = (g(1) + a1 eps64) sum|x - r|      (before the store)
        |out' - out| <= e_L1 (1 + eps32) + eps32 |out|                             (the store: one rounding)
    KL columns 5..7: c sum_d t_d with t = 1 + lv - mu^2 - expf(lv) in fp32 and c = -0.5 (exact) or -1.  1 + lv, mu^2, their
    difference and the last difference: no operand passes more than 4 roundings, expf has X of its own.  The four terms
    cancel (t = 0 at mu = lv = 0), so the bound is against the sum of their ABSOLUTE values, not against t:
        tol_t = g(4) (1 + |lv| + mu^2 + E) + X eps32 (1 + g(4)) E
        a2 = ceil(D / 256) + 26,          e_KL = |c| (sum tol_t + a2 eps64 sum|t|)
        |out' - out| <= e_KL (1 + eps32) + eps32 |out|.
    LOSS = mse_cof (((L1_1 + L1_2) + L1_1hat) + L1_2hat) + kl_cof (KL_1 + KL_2), in float64 from the UNROUNDED sums (mse_cof
    and kl_cof are the fp32 values passed): the parts' errors before their stores, weighted, three + one + two float64
    additions / products on top (8 eps64 of the absolute terms covers them), one rounding at the store:
        |out0' - out0| <= (|mse_cof| sum e_L1 + |kl_cof| (e_KL1 + e_KL2) + 8 eps64 A) (1 + eps32) + eps32 |out0|,
        A = |mse_cof| sum L1 + |kl_cof| (|KL_1| + |KL_2|).
group_sum_f64: pure float64 additions in row order starting from what the buffer held: the sequential numpy statement below
    gives the same bits; no bound.
"""
import numpy as np

from elem_ref import EPS32, EPS64, EXPF_ROUNDINGS, FLOOR, g

X = EXPF_ROUNDINGS
F64, F32 = np.float64, np.float32
TERMS = ("LOSS", "L1_1", "L1_2", "L1_1hat", "L1_2hat", "KL_1", "KL_2", "KL_style")
WG = 256                      # threads of a pair's workgroup (csrc/val.hip)


def uses_float4(n_per, aligned=True):
    """The path dvae_pair_metrics takes: float4 loads when the four mel operands are 16-byte aligned and n_per % 4 == 0."""
    return bool(aligned) and n_per % 4 == 0


def thread_trips(n_per, aligned=True):
    """Loop trips of the busiest thread over the mel elements."""
    n = n_per // 4 if uses_float4(n_per, aligned) else n_per
    return -(-n // WG)


def kl_terms(mu, lv):
    mu, lv = np.asarray(mu, F64), np.asarray(lv, F64)
    return 1.0 + lv - mu * mu - np.exp(lv)


def tol_term(mu, lv):
    mu, lv = np.asarray(mu, F64), np.asarray(lv, F64)
    E = np.exp(lv)
    return g(4) * (1.0 + np.abs(lv) + mu * mu + E) + X * EPS32 * (1 + g(4)) * E


def _shapes(x1, x2, rec, rec_hat, q_mu, q_lv, s_mu, s_lv):
    Bh = np.shape(x1)[0]
    f = lambda a, rows: np.asarray(a, F64).reshape(rows, -1)
    return (Bh, f(x1, Bh), f(x2, Bh), f(rec, 2 * Bh), f(rec_hat, 2 * Bh), f(q_mu, 2 * Bh), f(q_lv, 2 * Bh), f(s_mu, Bh),
            f(s_lv, Bh))


def pair_rows(x1, x2, rec, rec_hat, q_mu, q_lv, s_mu, s_lv, mse_cof, kl_cof):
    """out [Bh, 8] in float64: loss_functionGVAE2 of every pair on its own (batch_size = 1), layouts of forward_full."""
    Bh, x1, x2, rec, rec_hat, q_mu, q_lv, s_mu, s_lv = _shapes(x1, x2, rec, rec_hat, q_mu, q_lv, s_mu, s_lv)
    out = np.zeros((Bh, 8), F64)
    out[:, 1] = np.abs(x1 - rec[:Bh]).sum(1)
    out[:, 2] = np.abs(x2 - rec[Bh:]).sum(1)
    out[:, 3] = np.abs(x1 - rec_hat[:Bh]).sum(1)
    out[:, 4] = np.abs(x2 - rec_hat[Bh:]).sum(1)
    kl = kl_terms(q_mu, q_lv).sum(1)
    out[:, 5], out[:, 6] = -0.5 * kl[:Bh], -0.5 * kl[Bh:]
    out[:, 7] = -kl_terms(s_mu, s_lv).sum(1)
    mse, klc = float(F32(mse_cof)), float(F32(kl_cof))
    out[:, 0] = mse * (((out[:, 1] + out[:, 2]) + out[:, 3]) + out[:, 4]) + klc * (out[:, 5] + out[:, 6])
    return out


def pair_bounds(x1, x2, rec, rec_hat, q_mu, q_lv, s_mu, s_lv, mse_cof, kl_cof):
    """(reference rows [Bh, 8], bound [Bh, 8]) of one dvae_pair_metrics launch."""
    ref = pair_rows(x1, x2, rec, rec_hat, q_mu, q_lv, s_mu, s_lv, mse_cof, kl_cof)
    Bh, x1, x2, rec, rec_hat, q_mu, q_lv, s_mu, s_lv = _shapes(x1, x2, rec, rec_hat, q_mu, q_lv, s_mu, s_lv)
    n_per, D, S = x1.shape[1], q_mu.shape[1], s_mu.shape[1]
    e = np.zeros((Bh, 8), F64)                     # the errors before the store
    a1 = -(-n_per // WG) + 28
    e[:, 1:5] = (g(1) + a1 * EPS64) * ref[:, 1:5]
    for col, mu, lv, c, n in ((5, q_mu[:Bh], q_lv[:Bh], 0.5, D), (6, q_mu[Bh:], q_lv[Bh:], 0.5, D), (7, s_mu, s_lv, 1.0, S)):
        a2 = -(-n // WG) + 26
        e[:, col] = c * (tol_term(mu, lv).sum(1) + a2 * EPS64 * np.abs(kl_terms(mu, lv)).sum(1))
    mse, klc = abs(float(F32(mse_cof))), abs(float(F32(kl_cof)))
    A = mse * ref[:, 1:5].sum(1) + klc * (np.abs(ref[:, 5]) + np.abs(ref[:, 6]))
    e[:, 0] = mse * e[:, 1:5].sum(1) + klc * (e[:, 5] + e[:, 6]) + 8 * EPS64 * A
    return ref, e * (1 + EPS32) + EPS32 * np.abs(ref) + FLOOR


def group_sum(rows, group, G, sums=None, counts=None, bad=None):
    """dvae_group_sum_f64, row by row: (sums [G + 1, K] float64, counts [G + 1], bad [G + 1] int64), accumulated into the
    arrays given (copies are returned).  Row G is the total; a row with a value that is not finite adds to bad[its group] and
    bad[G], a row whose group is out of range to bad[G] alone; neither enters a sum."""
    rows = np.asarray(rows, F32)
    P, K = rows.shape
    sums = np.zeros((G + 1, K), F64) if sums is None else np.array(sums, F64)
    counts = np.zeros(G + 1, np.int64) if counts is None else np.array(counts, np.int64)
    bad = np.zeros(G + 1, np.int64) if bad is None else np.array(bad, np.int64)
    for p in range(P):
        gp = int(group[p])
        if not 0 <= gp < G:
            bad[G] += 1
        elif not np.isfinite(rows[p]).all():
            bad[gp] += 1
            bad[G] += 1
        else:
            for dst in (gp, G):
                sums[dst] = sums[dst] + rows[p].astype(F64)          # one float64 addition per column, in row order
                counts[dst] += 1
    return sums, counts, bad


# ------------------------------------------------------------------ inputs of the tests (CPU and GPU alike)
def pair_inputs(Bh, n_per, D, S, seed):
    """Inputs in the model's ranges: mels U[0, 1) (reconstructions a little outside), mu ~ N(0, 1), lv in [-6, 2]."""
    rs = np.random.RandomState(seed)
    u = lambda *s: rs.uniform(0.0, 1.0, s).astype(F32)
    d = {"x1": u(Bh, n_per), "x2": u(Bh, n_per),
         "rec": (u(2 * Bh, n_per) + rs.uniform(-0.1, 0.1, (2 * Bh, n_per))).astype(F32),
         "rec_hat": (u(2 * Bh, n_per) + rs.uniform(-0.1, 0.1, (2 * Bh, n_per))).astype(F32),
         "q_mu": rs.standard_normal((2 * Bh, D)).astype(F32), "q_lv": rs.uniform(-6, 2, (2 * Bh, D)).astype(F32),
         "s_mu": rs.standard_normal((Bh, S)).astype(F32), "s_lv": rs.uniform(-6, 2, (Bh, S)).astype(F32)}
    d["rec"][0, 0] = d["x1"][0, 0]                 # a tie, and the last element keeps a full difference: a lost tail shows
    d["rec_hat"][-1, -1] = d["x2"][-1, -1] + F32(0.5)
    return d


KEYS = ("x1", "x2", "rec", "rec_hat", "q_mu", "q_lv", "s_mu", "s_lv")
N_PER = [1, 3, 4, 1020, 1024, 1028, 5120]         # scalar path, one float4, either side of one 256-thread trip, 80 x 64
BH = [1, 3]
D = [1, 32, 257]                                  # one thread, the model's latent width, a second trip of one thread
S = [1, 4]
