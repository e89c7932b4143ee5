"""The float64 restatement of the scheduled loss (dvae_loss_fwd_sched / dvae_loss_bwd_sched of csrc/elem.hip: the two weights
read from the device, per-dimension free bits) and the rounding bounds one launch is held to.  Not a test module:
tests/test_kl_sched_ref.py proves it on the CPU, tests/test_hip_kl_sched.py holds the kernels to it.  Everything that is not
new here is elem_ref's, by import: the formulas of the eight terms, the bound of one KL term, the inputs.

Definitions (include/dvae_hip.h), q*_mu / q*_lv row-major [rows, D], lambda = free_bits:
    kl_dim_k[j] = kl_scale sum_i t_ij,   t = 1 + lv - mu^2 - exp(lv),   kl_scale = -0.5 / rows
    gate_k[j]   = kl_dim_k[j] > lambda[j]            (strict; all ones without free bits)
    aux[k]      = sum_j max(lambda[j], kl_dim_k[j])  (without free bits: out8[5 + k] itself)
    out8[0]     = coef[0] (((t1 + t2) + t3) + t4) + coef[1] (aux[0] + aux[1]);   out8[1..7]: elem_ref.loss_fwd's
    backward, element (i, j) of half k:  W = (g0 coef[1] gate_k[j] + g[5 + k]) kl_scale,  dmu = W (-2 mu),  dlv = W (1 - exp lv)

Bounds (elem_ref's notation: eps32, eps64, g(k), FLOOR, tol_term the bound of one fp32 term):
kl_dim: a thread adds the `rows` terms of its column in float64 in row order, multiplies by the scale and rounds once;
    16 more float64 roundings for the reference's own pairwise sum:   a = rows + 17,
        |kd' - kd| <= |kl_scale| (sum_i tol_term_ij + a eps64 sum_i |t_ij|) (1 + eps32) + eps32 |kd|          (tol_kd)
aux[k] with free bits: the D values max(lambda_j, kd'_j) of the DEVICE's fp32 kl_dim added in float64 in dimension order, one
    rounding.  max(lambda, .) moves by no more than its argument does, and the gate is the reference's own (below), so
        |aux' - aux| <= sum_j tol_kd[j] + (D + 16) eps64 sum_j |max(lambda_j, kd_j)| (1 + eps32) + eps32 |aux|
    Without free bits aux[k] is out8[5 + k]: elem_ref.kl_fwd_bounds.
out8[0] from the device's OWN out8[1..4] and aux[0..1] (inputs, not errors), as elem_ref bounds it:
        g(5) (|coef0| sum |t_1..4| + |coef1| (|aux0| + |aux1|)).
gradients: elem_ref.loss_bwd_bounds with mse_cof = coef[0], kl_cof = coef[1] on a penalised dimension; on a free one the
    weight is g[5 + k] kl_scale (the same statement with g0 = 0: fewer roundings, the same bound formula).
The gate is a comparison: a column whose mean sits on lambda could flip under rounding.  `free_bits_for` chooses lambda so
that NO column has |kl_dim - lambda| below MARGIN = 10 times that column's tol_kd, in either half, and asserts it: the
device's gate must then equal the reference's exactly, and so must the free counts.
"""
import numpy as np

import elem_ref as E

F32, F64 = np.float32, np.float64
EPS32, EPS64, FLOOR, g = E.EPS32, E.EPS64, E.FLOOR, E.g
MARGIN = 10.0
LOSS_MAX_D = 1024          # DVAE_LOSS_MAX_D of include/dvae_hip.h

# (rows, D): one row, one column, the model's own (batch 4 and 64 at latent_dim 32 / 64), more columns than one pass of 256
# threads, more rows than threads, the largest D, neither a multiple of anything
SHAPES = [(1, 1), (1, 32), (3, 5), (4, 32), (2, 64), (64, 64), (130, 5), (2, 1024), (300, 257)]
NS = [4, 1023]             # elements of the L1 part (covered by tests/test_hip_elem.py: a tail-only and a ragged size here)


def divisors(nq):
    """The D the bit-equality cases run an nq with: 1, nq itself and one in between where there is one (255 = 5 x 51)."""
    return sorted({1, nq} | {D for D in (5,) if nq % D == 0 and D <= LOSS_MAX_D})


def bit_cases():
    """(n, nq, ns) of elem_ref.CASES: every L1 size with every latent size."""
    return [(n, nq, ns) for n in E.CASES["l1"] for nq, ns in E.CASES["loss_nq_ns"]]


def inputs(rows, D, n, seed, ns=7):
    """elem_ref.loss_inputs for q blocks [rows, D] with log-variances of the order of the other terms, kl_scale = -0.5 / rows."""
    d = E.loss_inputs(n, rows * D, ns, "R", seed, wide=False)
    d["kl_scale"] = F32(-0.5 / rows)
    d["rows"], d["D"] = rows, D
    if rows * D == 1:          # the one element is elem_ref's edge mu = lv = 0, which has no KL to gate on
        d["q1_mu"][0], d["q2_mu"][0] = F32(1.0), F32(-1.5)
    return d


def positive_inputs(rows, D, n, seed):
    """`inputs` with every |mu| >= 0.25: each element's KL is at least mu^2 / 2 > 0.03, so lambda = 0 gates every dimension on
    with a margin."""
    d = inputs(rows, D, n, seed)
    for k in ("q1_mu", "q2_mu"):
        d[k] = np.where(np.abs(d[k]) < 0.25, F32(0.5), d[k]).astype(F32)
    return d


def kl_dim(d):
    """[2, D] float64: the batch-mean KL per dimension of z1, z2."""
    s = float(F32(d["kl_scale"]))
    return np.stack([E.kl_terms(d[m], d[l]).reshape(d["rows"], d["D"]).sum(0) * s
                     for m, l in (("q1_mu", "q1_lv"), ("q2_mu", "q2_lv"))])


def tol_kl_dim(d):
    s, a = abs(float(F32(d["kl_scale"]))), d["rows"] + 17
    out = []
    for m, l in (("q1_mu", "q1_lv"), ("q2_mu", "q2_lv")):
        t = np.abs(E.kl_terms(d[m], d[l])).reshape(d["rows"], d["D"]).sum(0)
        tt = E.tol_term(d[m], d[l]).reshape(d["rows"], d["D"]).sum(0)
        out.append(s * (tt + a * EPS64 * t) * (1 + EPS32))
    kd = kl_dim(d)
    return np.stack(out) + EPS32 * np.abs(kd) + FLOOR


def free_bits_for(d, single="free"):
    """lambda [D] fp32: even dimensions free in both halves (twice the larger mean, and a little), odd ones penalised in both
    (half the smaller mean); a dimension whose smaller mean is too close to zero for the margin is made free instead.  D == 1:
    `single` says which way.  Asserts the margin and (D > 1) one free and one penalised dimension in each half."""
    kd, tol = kl_dim(d), tol_kl_dim(d)
    D = d["D"]
    hi, lo = kd.max(0), kd.min(0)
    free = (np.arange(D) % 2 == 0) if D > 1 else np.array([single == "free"])
    lam_on = F32(0.5) * lo.astype(F32)
    ok_on = np.all(np.abs(kd - lam_on.astype(F64)) >= 2 * MARGIN * tol, 0) & np.all(kd > lam_on.astype(F64), 0)
    assert D > 1 or free[0] or ok_on[0], "the single column cannot be penalised with a margin"
    free = free | ~ok_on
    lam = np.where(free, (2.0 * hi + 0.125).astype(F32), lam_on).astype(F32)
    check_margin(d, lam)
    gate = kd > lam.astype(F64)
    if D > 1:
        assert gate.any(1).all() and (~gate).any(1).all(), "each half needs a free and a penalised dimension"
    return lam


def check_margin(d, lam):
    kd, tol = kl_dim(d), tol_kl_dim(d)
    gap = np.abs(kd - np.asarray(lam, F64)[None, :])
    assert (gap >= MARGIN * tol).all(), f"a column sits within {MARGIN} bounds of its lambda: {float((gap / tol).min()):.3g}"


def fwd(d, coef, lam=None):
    """(out8, aux) in float64; aux = [aux0, aux1, free1, free2, kl_dim (2 D), gate (2 D)]."""
    c0, c1 = float(F32(coef[0])), float(F32(coef[1]))
    out = E.loss_fwd(dict(d, mse_cof=F32(c0), kl_cof=F32(c1)))
    kd, D = kl_dim(d), d["D"]
    if lam is None:
        gate, a, nfree = np.ones((2, D)), out[5:7].copy(), np.zeros(2)
    else:
        lam64 = np.asarray(lam, F32).astype(F64)
        gate = (kd > lam64[None, :]).astype(F64)
        a, nfree = np.maximum(kd, lam64[None, :]).sum(1), (1.0 - gate).sum(1)
    out[0] = c0 * (out[1] + out[2] + out[3] + out[4]) + c1 * (a[0] + a[1])
    return out, np.concatenate([a, nfree, kd.reshape(-1), gate.reshape(-1)])


def bwd(d, coef, g8, gate=None, dt=F64, ex=np.exp):
    """The ten gradients in the order of dvae_loss_bwd_sched's arguments; gate [2, D] of `fwd` (None: all ones)."""
    dd = dict(d, mse_cof=F32(coef[0]), kl_cof=F32(coef[1]))
    out = E.loss_bwd(dd, g8, dt, ex)
    if gate is None:
        return out
    g0 = np.asarray(g8, dt).copy()
    g0[0] = 0
    free = E.loss_bwd(dd, g0, dt, ex)           # the weight of a free dimension: nothing from g8[0]
    on = np.tile(np.asarray(gate, F64) != 0, (1, d["rows"])).reshape(2, d["rows"] * d["D"])
    for k in range(2):
        for j in (4 + 2 * k, 5 + 2 * k):
            out[j] = np.where(on[k], out[j], free[j])
    return out


def fwd_bounds(d, coef, lam=None, dev_out=None, dev_aux=None):
    """(out8, aux, tol_out8, tol_aux); with the device's own out8 and aux, out8[0] and its bound come from them."""
    out, aux = fwd(d, coef, lam)
    D = d["D"]
    c0, c1 = abs(float(F32(coef[0]))), abs(float(F32(coef[1])))
    _, tol8 = E.loss_fwd_bounds(dict(d, mse_cof=F32(coef[0]), kl_cof=F32(coef[1])))
    tkd = tol_kl_dim(d)
    taux = np.zeros_like(aux)
    taux[4:4 + 2 * D] = tkd.reshape(-1)
    if lam is None:
        taux[0:2] = tol8[5:7]
    else:
        m = np.abs(np.maximum(kl_dim(d), np.asarray(lam, F32).astype(F64)[None, :]))
        taux[0:2] = tkd.sum(1) + (D + 16) * EPS64 * m.sum(1) * (1 + EPS32) + EPS32 * np.abs(aux[0:2]) + FLOOR
    if dev_out is not None:
        t, a = np.asarray(dev_out, F64), np.asarray(dev_aux, F64)
        cc0, cc1 = float(F32(coef[0])), float(F32(coef[1]))
        out[0] = cc0 * (t[1] + t[2] + t[3] + t[4]) + cc1 * (a[0] + a[1])
        tol8[0] = g(5) * (c0 * np.abs(t[1:5]).sum() + c1 * (abs(a[0]) + abs(a[1]))) + FLOOR
    else:
        tol8[0] = g(5) * (c0 * np.abs(out[1:5]).sum() + c1 * np.abs(aux[0:2]).sum()) + c1 * taux[0:2].sum() + c0 * tol8[1:5].sum() + FLOOR
    return out, aux, tol8, taux


def bwd_bounds(d, coef, g8, gate=None):
    """(reference gradients, bounds), as elem_ref.loss_bwd_bounds; a free dimension is bounded with g8[0] = 0."""
    dd = dict(d, mse_cof=F32(coef[0]), kl_cof=F32(coef[1]))
    g8 = np.asarray(g8, F32)
    ref = bwd(d, coef, g8.astype(F64), gate)
    _, tol = E.loss_bwd_bounds(dd, g8)
    if gate is not None:
        g0 = g8.copy()
        g0[0] = 0
        _, tfree = E.loss_bwd_bounds(dd, g0)
        on = np.tile(np.asarray(gate, F64) != 0, (1, d["rows"])).reshape(2, d["rows"] * d["D"])
        for k in range(2):
            for j in (4 + 2 * k, 5 + 2 * k):
                tol[j] = np.where(on[k], tol[j], tfree[j])
    return ref, tol


def fwd_f32(d, coef, lam, push=0):
    """The kernel's statement of kl_dim and aux[0..3]: fp32 terms (an exp wrong by up to elem_ref's X roundings towards
    `push`), float64 over the rows, one rounding; the clamped sum over the rounded values in float64, one rounding."""
    ex, s = E.exp32(push), float(F32(d["kl_scale"]))
    kd = np.stack([(E.kl_terms(d[m], d[l], F32, ex).astype(F64).reshape(d["rows"], d["D"]).sum(0) * s).astype(F32)
                   for m, l in (("q1_mu", "q1_lv"), ("q2_mu", "q2_lv"))])
    lam = np.asarray(lam, F32)
    gate = kd > lam[None, :]
    a = np.where(gate, kd, lam[None, :]).astype(F64).sum(1).astype(F32)
    return kd, gate, a
