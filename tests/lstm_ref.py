"""The float64 reference of the LSTM recurrence kernels (csrc/lstm.hip, csrc/lstm_pers.hip: every kernel behind
dvae_lstm_seq_fwd / _bwd / _fwd_range / _bwd_range) and the bounds one FRAME is held to.  Not a test module:
tests/test_lstm_ref.py proves the reference against torch.nn.LSTM in float64 and the bounds against an fp32 restatement of
the kernels on the CPU, tests/test_hip_lstm.py holds the kernels to both.  A change here moves what the GPU tests accept: the
formulas are the kernels', the bounds are derived below, neither follows what some code computes.

Gate order i, f, g, o (rows qH + j of W_hh [4H, H], columns qH + j of gates / dgates [T, N, 4H]).  `reverse` as in
dvae_lstm_dir_t: the recurrence visits t = T-1 .. 0.  In recurrence order frame t follows tp and precedes tn.

Teacher-forced frames.  A frame is judged from the DEVICE'S OWN neighbours: forward frame t from the h'[tp], c'[tp] the
device stored (zeros at the first frame) and its own activated gates; backward frame t from the device's own gates, c_all and
dgates'[tn] (and its own dc_ws where the launch can be stepped).  A stale or mis-addressed hand-off between frames or
workgroups shows as a frame that does not follow from its stored predecessor.  Operands as the mode takes them: fp32 and
fp32x3 as stored; bf16 mode: W_hh and the recurrent operand (h[tp], dG[tn]) rounded to bf16 (RNE) first.

The bounds.  eps32 = 2^-24 is one fp32 rounding, g(k) = k eps32 / (1 - k eps32) is k of them compounded, FLOOR = 2^-126.

recurrent product (tol_a, tol_dh)
    a_q = x_q + sum_k W[qH+j, k] h'[tp][n, k],  A_q = |x_q| + sum |W| |h'|   (backward: dh = dh_out + sum_k dG'[tn][n, k]
    W[k, j], K = 4H, A likewise).  A worst-case g(K) A is useless at K = 1024 .. 4096, so the error is MEASURED against a
    reference: `seq_dot` is a plain left-to-right fp32 dot product of the same operands with two roundings per term
    (product, sum), then the addition of x (dh_out), run on a fixed sample of columns holding the first and last unit of
    every 16-unit tile of every gate (every column while N H <= 8192: `sample_units`).  The fp32 MFMA is a k-ordered fmaf chain (one rounding per term) and no kernel has a
    chain longer than K, so that emulation is an upper reference.  Per frame rho_max, rho_rms = its worst and RMS |err| / A
    against float64.  The device must keep   |err| <= 2 rho_max A  at every element   and   RMS |err| / A <= 2 rho_rms  over
    the frame  (the factor 2: the order inside the bf16 MFMAs is not documented; two same-length chains in different orders
    differ by about that).  Neither a nor dh is stored, so the first condition enters every stored quantity as tol_a = 2
    rho_max A (tol_dh), and the second is held through a LOWER bound of the device's |err|: for a gate,
    r = max(|q' - act(a)| - C_act eps32, 0) / L <= |a' - a|  (L: the activation's largest slope over [a - tol_a, a + tol_a]),
    taken over the elements of the frame where the stored value still tells the error: the tanh gate where L >= 0.5 (a set
    fixed by the float64 a; at a sigmoid's slope of 1/4 or less C_act eps32 / L alone exceeds the errors in question, and a
    lost split term at K = 1024 would hide behind it).  For dh, r = max(|dG_o' - dG_o| - tol_o(tol_dh = 0), 0) / |tc o (1 - o)|
    from the o-gate gradient, which is linear in dh, over the whole frame.  RMS(r / A) <= 2 rho_rms is what is asserted: a
    device that keeps the condition keeps this.
gates
    |q' - act(a_q)| <= L tol_a + C_act eps32,  C_act = GATE_SIGMOID_ABS / GATE_TANH_ABS: ABSOLUTE errors of gate_sigmoid /
    gate_tanh (csrc/common.h) in units of eps32, measured (scripts/probes/gate_sweep.hip) — both expressions cancel by
    design: 1 - 2 rcp(e^2x + 1) is accurate absolutely, not relative to tanh x near 0.  Where |a| - tol_a >= 90 the gate must
    be EXACTLY 0, 1 or -1 (the probe found every |x| >= 90 so), where a == 0 exactly gate_tanh must give exactly 0.
c   against f' c'[tp] + i' g' from the device's own gates: two products and a sum, |err| <= g(3) (|f' c'| + |i' g'|).
h   against o' tanh(c'):  |err| <= |o'| GATE_TANH_ABS eps32 + eps32 |h|  (the product), + 2^-8 (|h| + tol) where h is stored as
    bf16: bf16 keeps 8 significant bits, so round-to-nearest-even moves a value by up to 2^-8 of itself (half a unit in the last
    place of a value just above a power of two).  2^-9 is NOT a bound of a correctly rounded store: the fp32 restatement of
    tests/test_lstm_ref.py, whose bf16 store is exact RNE, reaches 1.99 x 2^-9.
backward epilogue (lstm.hip: lstm_step_bwd_kernel; every kernel has the same statement)
        tc = gate_tanh(c);  dc = dcar + dh o (1 - tc^2);  dG_i = dc g i (1 - i);  dG_f = dc c[tp] f (1 - f);
        dG_g = dc i (1 - g^2);  dG_o = dh tc o (1 - o);  dcar' = dc f
    from the device's own i, f, g, o, c, c[tp] (exact inputs).  Every factor carries (value, absolute tolerance):
        dh: tol_dh;   tc: dt = GATE_TANH_ABS eps32;
        1 - tc^2: 2 |tc| dt + dt^2 (propagation) + eps32 (|tc| + dt)^2 (the square) + eps32 |1 - tc^2| (the difference) —
            absolute, NOT relative to 1 - tc^2, which cancels at saturation;
        1 - s (s = i, f, o): eps32 |1 - s| (one rounding of exact inputs);  1 - g^2: eps32 (g^2 + |1 - g^2|).
    A product of factors (v_i, d_i) with k multiplications:  |err| <= prod(|v_i| + d_i) - prod|v_i| + g(k) prod(|v_i| + d_i)
    (`_prod`: full-order propagation plus k roundings).  dc = dcar + v:  tol_dc = tol_car + tol_v + eps32 (|dcar| + |v| +
    tol_car + tol_v).  bf16-stored dG: + 2^-8 (|dG| + tol).
the cell-gradient carry
    Stepped launches (H % 512 == 0, per-frame kernels, dvae_lstm_seq_bwd_range(step, step + 1)): dc_ws is read after every
    step, the next frame takes the device's own (tol_car = 0).  Whole-sequence launches: the reference carries its own
    float64 dcar' = dc f' with tol_car' = the product bound of (dc, tol_dc) x f'  (= |f'| tol_dc (1 + eps32) + eps32 |dcar'|
    to first order).  The last dc_ws is held to the same bound where the kernel stores it.
bias gradients of the persistent backward launch
    Per column, against the float64 column sum s of the device's own dgates; a row group sums its T * (rows) terms and 16
    lanes' shares in fp32: g(T N + 16) sum|dG'| covers every order.
    dbias_part: the float64 sum of the 16 slabs against s:  g(T N + 16) sum|dG'| + eps32 |s|; rows of row groups the launch
    cannot have (>= ceil(N/16)) are exactly 0.
    dbias_ih / dbias_hh: against old + s.  Every row group ADDS its share to the accumulator with one fp32 atomic
    (pers_bias_out), so the running value old + (shares so far) is rounded once per row group, not once:
        g(T N + 16) sum|dG'| + n_rb eps32 (|old| + sum|dG'|),     n_rb <= ceil(N/16) row groups.
    (One rounding, eps32 |result|, holds for a single row group only: with old in +-2 and a column whose gradients are tiny
    — a saturated unit — the launches of 3, 5 and 7 row groups measured 1.3, 2.4 and 2.4 eps32 |result|.)
"""
import collections
import zlib

import numpy as np

from ref_common import (BF16_REL, EPS32, F, F64, FLOOR, MODE_BF16, MODE_F32, MODE_F32X3, bf16, fma as _fma, g, split3,  # noqa: F401
                        worst_ratio)

# gate_sigmoid / gate_tanh of csrc/common.h against float64, worst |err| / 2^-24 over 40 000 001 evenly spaced x in
# [-100, 100] and 2^23 log-spaced |x| in [1e-6, 100] of either sign on the MI355X (scripts/probes/gate_sweep.hip; DESIGN.md
# section 5):  gate_sigmoid 1.8503 (at x = 3.60230398),  gate_tanh 3.6663 (at x = -1.78888464); nothing non-finite, every
# |x| >= 90 exactly 0 / 1 / +-1, gate_tanh(0) == 0.  (Relative to tanh x the error of gate_tanh reaches 8.6 % at
# x = 1.04e-6.)  The sweep is a sample: the bounds are twice the measured worst.
GATE_SIGMOID_MEASURED = 1.8503
GATE_TANH_MEASURED = 3.6663
GATE_SIGMOID_ABS = 2.0 * GATE_SIGMOID_MEASURED
GATE_TANH_ABS = 2.0 * GATE_TANH_MEASURED
SATURATED = 90.0                 # |x| from which the probe found both gate functions exact


def operand(v, mode):
    """The operand of the recurrent product as the mode takes it (float32 values)."""
    return bf16(v) if mode == MODE_BF16 else np.asarray(v, F)


def sigmoid(x):
    x = np.asarray(x, F64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def sample_units(H, N):
    """The units the sequential emulation runs on: the first and last of every 16-unit tile; every unit while N H <= 8192
    (the worst of a few hundred samples is too noisy a yardstick for a frame of as many elements)."""
    return np.arange(H) if N * H <= 8192 else np.array([16 * b + e for b in range(H // 16) for e in (0, 15)])


def sample_cols(H, N):
    """... of every gate: columns of [*, 4H]."""
    return np.concatenate([q * H + sample_units(H, N) for q in range(4)])


def seq_dot(a, b, add=None):
    """Plain left-to-right fp32 dot products a [N, K] x b [K, M]: two roundings per term, then + add."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    acc = np.zeros((a.shape[0], b.shape[1]), F)
    for k in range(a.shape[1]):
        acc += a[:, k:k + 1] * b[k]
    return acc if add is None else acc + np.asarray(add, F)


def rho(emul, ref, A):
    """(worst, RMS) of |emul - ref| / A; 0 where A == 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(A > 0, np.abs(np.asarray(emul, F64) - ref) / A, 0.0)
    return (float(r.max()), float(np.sqrt((r * r).mean()))) if r.size else (0.0, 0.0)


def _prod(factors, k):
    """Product of (value, absolute tolerance) factors with k fp32 multiplications: (value, bound)."""
    v, hi = 1.0, 1.0
    for val, tol in factors:
        v = v * val
        hi = hi * (np.abs(val) + tol)
    return v, np.maximum(hi - np.abs(v), 0.0) + g(k) * hi + FLOOR


# ------------------------------------------------------------------ the frame, float64
def fwd_math(a, c_prev):
    """(gates [N, 4H], c, h) from pre-activations a [N, 4H] and c_prev [N, H]."""
    H = a.shape[1] // 4
    i, f, o = sigmoid(a[:, :H]), sigmoid(a[:, H:2 * H]), sigmoid(a[:, 3 * H:])
    gg = np.tanh(a[:, 2 * H:3 * H])
    c = f * c_prev + i * gg
    return np.concatenate([i, f, gg, o], 1), c, o * np.tanh(c)


def bwd_math(dh, dcar, gates, c, c_prev):
    """(dgates [N, 4H], dcar') of one frame, the kernels' epilogue in float64."""
    H = c.shape[1]
    i, f, gg, o = (np.asarray(gates[:, q * H:(q + 1) * H], F64) for q in range(4))
    tc = np.tanh(c)
    dc = dcar + dh * o * (1.0 - tc * tc)
    dG = np.concatenate([dc * gg * i * (1.0 - i), dc * c_prev * f * (1.0 - f), dc * i * (1.0 - gg * gg),
                         dh * tc * o * (1.0 - o)], 1)
    return dG, dc * f


def order(T, reverse):
    """Frames in recurrence order."""
    return list(range(T - 1, -1, -1)) if reverse else list(range(T))


def run_fwd(x, W, reverse):
    """Free-running float64 forward pass: (gates, c, h), each [T, N, *]."""
    x, W = np.asarray(x, F64), np.asarray(W, F64)
    T, N, H4 = x.shape
    gates, c, h = np.zeros((T, N, H4)), np.zeros((T, N, H4 // 4)), np.zeros((T, N, H4 // 4))
    hp, cp = np.zeros((N, H4 // 4)), np.zeros((N, H4 // 4))
    for t in order(T, reverse):
        gates[t], c[t], h[t] = fwd_math(x[t] + hp @ W.T, cp)
        hp, cp = h[t], c[t]
    return gates, c, h


def run_bwd(dh_out, W, gates, c, reverse, carry=True):
    """Free-running float64 backward pass: (dgates [T, N, 4H], last dcar)."""
    W = np.asarray(W, F64)
    T, N, H = c.shape
    dG, dcar, rec = np.zeros((T, N, 4 * H)), np.zeros((N, H)), np.zeros((N, H))
    o = order(T, reverse)
    for s in range(T - 1, -1, -1):
        t = o[s]
        cp = c[o[s - 1]] if s > 0 else np.zeros((N, H))
        dG[t], dcar = bwd_math(np.asarray(dh_out[t], F64) + rec, dcar, gates[t], c[t], cp)
        if not carry:
            dcar = np.zeros((N, H))
        rec = dG[t] @ W
    return dG, dcar


# ------------------------------------------------------------------ one frame of the device against the reference
def act_bounds(a, tol_a, H):
    """(act(a), largest slope over [a - tol_a, a + tol_a], C_act) per column of [N, 4H]."""
    near = np.maximum(np.abs(a) - tol_a, 0.0)
    s = sigmoid(near)
    with np.errstate(over="ignore"):
        slope = np.concatenate([(s * (1 - s))[:, :2 * H], (1.0 / np.cosh(near[:, 2 * H:3 * H]) ** 2), (s * (1 - s))[:, 3 * H:]], 1)
    ref = np.concatenate([sigmoid(a[:, :2 * H]), np.tanh(a[:, 2 * H:3 * H]), sigmoid(a[:, 3 * H:])], 1)
    C = np.concatenate([np.full(2 * H, GATE_SIGMOID_ABS), np.full(H, GATE_TANH_ABS), np.full(H, GATE_SIGMOID_ABS)])
    return ref, slope, C


def fwd_frame(x, W, h_prev, c_prev, gates, c, h, mode, h_bf16=False):
    """Forward frame: x [N, 4H] fp32 pre-activations, W [4H, H], the device's h'[tp], c'[tp] (None at the first frame) and what
    it stored for this frame.  Returns {name: (worst error / bound, flat index)}; 'a_rms' and 'exact' have index -1."""
    x64 = np.asarray(x, F64)
    N, H = x64.shape[0], x64.shape[1] // 4
    gates, c, h = np.asarray(gates, F64), np.asarray(c, F64), np.asarray(h, F64)
    if h_prev is None:
        a, A, rmax, rrms = x64, np.abs(x64), 0.0, 0.0
        c_prev = np.zeros((N, H))
    else:
        Wm, hm = operand(W, mode), operand(h_prev, mode)
        a = x64 + hm.astype(F64) @ Wm.astype(F64).T
        A = np.abs(x64) + np.abs(hm).astype(F64) @ np.abs(Wm).astype(F64).T
        cols = sample_cols(H, N)
        rmax, rrms = rho(seq_dot(hm, Wm[cols].T, np.asarray(x, F)[:, cols]), a[:, cols], A[:, cols])
        c_prev = np.asarray(c_prev, F64)
    tol_a = 2.0 * rmax * A
    ref, slope, C = act_bounds(a, tol_a, H)
    out = {"gates": worst_ratio(gates, ref, slope * tol_a + C * EPS32 + FLOOR)}
    # the RMS condition through a lower bound of the device's |a' - a| (module docstring)
    # over the elements where a stored value still tells the error: the tanh gate at a slope of 0.5 or more (elsewhere
    # C_act eps32 / L is larger than the error in question); the set follows from the reference a alone
    gcol = slice(2 * H, 3 * H)
    lev = (slope[:, gcol] >= 0.5) & (A[:, gcol] > 0)
    num = np.maximum(np.abs(gates - ref)[:, gcol] - GATE_TANH_ABS * EPS32, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (num / slope[:, gcol] / A[:, gcol])[lev]
    rms = float(np.sqrt((r * r).mean())) if r.size else 0.0
    out["a_rms"] = ((0.0 if rms == 0.0 else rms / (2.0 * rrms) if rrms > 0 else np.inf), -1)
    # exact values: saturation and the zero of gate_tanh
    sat = np.abs(a) - tol_a >= SATURATED
    want = np.where(a > 0, 1.0, np.concatenate([np.zeros((N, 2 * H)), -np.ones((N, H)), np.zeros((N, H))], 1))
    bad = int((sat & (gates != want)).sum()) + int(((a[:, 2 * H:3 * H] == 0) & (gates[:, 2 * H:3 * H] != 0)).sum())
    bad += int((~np.isfinite(gates)).sum() + (~np.isfinite(c)).sum() + (~np.isfinite(h)).sum())
    out["exact"] = (np.inf if bad else 0.0, -1)
    i, f, gg, o = (gates[:, q * H:(q + 1) * H] for q in range(4))
    out["c"] = worst_ratio(c, f * c_prev + i * gg, g(3) * (np.abs(f * c_prev) + np.abs(i * gg)) + FLOOR)
    href = o * np.tanh(c)
    tol_h = np.abs(o) * GATE_TANH_ABS * EPS32 + EPS32 * np.abs(href) + FLOOR
    out["h"] = worst_ratio(h, href, tol_h + (BF16_REL * (np.abs(href) + tol_h) if h_bf16 else 0.0))
    out["tol_h"] = tol_h
    return out


def bwd_bounds(dh, tol_dh, dcar, tol_car, gates, c, c_prev, g_bf16=False):
    """References and bounds of the backward epilogue (module docstring): ((dG [N, 4H], tol), (dcar', tol))."""
    H = c.shape[1]
    i, f, gg, o = (np.asarray(gates[:, q * H:(q + 1) * H], F64) for q in range(4))
    tc, dt = np.tanh(c), GATE_TANH_ABS * EPS32
    u = 1.0 - tc * tc
    du = 2 * np.abs(tc) * dt + dt * dt + EPS32 * (np.abs(tc) + dt) ** 2
    du = du + EPS32 * (np.abs(u) + du)
    v, tol_v = _prod([(dh, tol_dh), (o, 0.0), (u, du)], 2)
    dc = dcar + v
    tol_dc = tol_car + tol_v + EPS32 * (np.abs(dcar) + np.abs(v) + tol_car + tol_v)
    one = lambda s: (1.0 - s, EPS32 * np.abs(1.0 - s))
    outs = [_prod([(dc, tol_dc), (gg, 0.0), (i, 0.0), one(i)], 3),
            _prod([(dc, tol_dc), (c_prev, 0.0), (f, 0.0), one(f)], 3),
            _prod([(dc, tol_dc), (i, 0.0), (1.0 - gg * gg, EPS32 * (gg * gg + np.abs(1.0 - gg * gg)))], 2),
            _prod([(dh, tol_dh), (tc, dt), (o, 0.0), one(o)], 3)]
    dG, tol = np.concatenate([p[0] for p in outs], 1), np.concatenate([p[1] for p in outs], 1)
    if g_bf16:
        tol = tol + BF16_REL * (np.abs(dG) + tol)
    return (dG, tol), _prod([(dc, tol_dc), (f, 0.0)], 1)


def bwd_frame(dh_out, W, dG_next, gates, c, c_prev, dcar, tol_car, dG, mode, g_bf16=False):
    """Backward frame: dh_out [N, H], W [4H, H], the device's dgates'[tn] (None at the first backward step), its gates, c,
    c[tp] (None at the first forward frame), the carry (the device's own with tol_car 0, or the reference's) and what the
    device stored.  Returns ({name: (ratio, index)}, (dcar', tol)) — the reference carry for the next frame."""
    dho = np.asarray(dh_out, F64)
    N, H = dho.shape
    c = np.asarray(c, F64)
    c_prev = np.zeros((N, H)) if c_prev is None else np.asarray(c_prev, F64)
    if dG_next is None:
        dh, A, rmax, rrms = dho, np.abs(dho), 0.0, 0.0
    else:
        Wm, gm = operand(W, mode), operand(dG_next, mode)
        dh = dho + gm.astype(F64) @ Wm.astype(F64)
        A = np.abs(dho) + np.abs(gm).astype(F64) @ np.abs(Wm).astype(F64)
        cols = sample_units(H, N)
        rmax, rrms = rho(seq_dot(gm, Wm[:, cols], np.asarray(dh_out, F)[:, cols]), dh[:, cols], A[:, cols])
    tol_dh = 2.0 * rmax * A
    (ref, tol), carry = bwd_bounds(dh, tol_dh, dcar, tol_car, gates, c, c_prev, g_bf16)
    dG = np.asarray(dG, F64)
    out = {"dgates": worst_ratio(dG, ref, tol)}
    (ref0, tol0), _ = bwd_bounds(dh, 0.0, dcar, tol_car, gates, c, c_prev, g_bf16)
    o = np.asarray(gates[:, 3 * H:], F64)
    lever = np.abs(np.tanh(c) * o * (1.0 - o))
    num = np.maximum(np.abs(dG[:, 3 * H:] - ref0[:, 3 * H:]) - tol0[:, 3 * H:], 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where((num > 0) & (lever > 0) & (A > 0), num / lever / A, 0.0)
    rms = float(np.sqrt((r * r).mean()))
    out["dh_rms"] = ((0.0 if rms == 0.0 else rms / (2.0 * rrms) if rrms > 0 else np.inf), -1)
    out["tol_dG"] = tol
    return out, carry


def check_dir(x, W, dh_out, reverse, mode, dev, h_bf16=False, g_bf16=False, dc_steps=None, passes="fb", tols=None):
    """Every frame of one direction.  dev: the device's gates [T, N, 4H], c, h [T, N, H] (h widened from bf16), and for the
    backward pass dG [T, N, 4H] and dc (the last dc_ws, or None where the kernel stores none); dc_steps: the device's dc_ws
    after each backward step (stepped launches) or None (the reference carries its own).  Returns {name: (worst ratio,
    'frame t index i')} over all frames.  tols: a dictionary that receives the bounds of h and dG, [T, N, *] (fp32 storage)."""
    T, N = x.shape[0], x.shape[1]
    H = x.shape[2] // 4
    o, res = order(T, reverse), {}

    def merge(d, t):
        for k in ("tol_h", "tol_dG"):
            v = d.pop(k, None)
            if v is not None and tols is not None:
                tols.setdefault(k, {})[t] = v
        for k, (r, i) in d.items():
            if k not in res or r > res[k][0]:
                res[k] = (r, f"frame {t} flat index {i}")

    if "f" in passes:
        for s, t in enumerate(o):
            tp = o[s - 1] if s else None
            merge(fwd_frame(x[t], W, None if tp is None else dev["h"][tp], None if tp is None else dev["c"][tp],
                            dev["gates"][t], dev["c"][t], dev["h"][t], mode, h_bf16), t)
    if "b" in passes:
        dcar, tol_car = np.zeros((N, H)), 0.0
        for s in range(T - 1, -1, -1):
            t, tp, tn = o[s], (o[s - 1] if s else None), (o[s + 1] if s + 1 < T else None)
            d, (dcar, tol_car) = bwd_frame(dh_out[t], W, None if tn is None else dev["dG"][tn], dev["gates"][t], dev["c"][t],
                                           None if tp is None else dev["c"][tp], dcar, tol_car, dev["dG"][t], mode, g_bf16)
            merge(d, t)
            if dc_steps is not None:                      # teacher-forced: the device's own dc_ws after this step
                merge({"dc": worst_ratio(dc_steps[T - 1 - s], dcar, tol_car)}, t)
                dcar, tol_car = np.asarray(dc_steps[T - 1 - s], F64), 0.0
        if dev.get("dc") is not None and dc_steps is None:       # (stepped: the last step's dc_ws has been judged above)
            merge({"dc": worst_ratio(dev["dc"], dcar, tol_car)}, o[0])
    return res


def bias_check(dG, old, got, slabs=None):
    """Bias gradients of a persistent backward launch from the device's own dgates [T, N, 4H]: `got` [4H] against old + the
    column sums, or `slabs` [16, 4H] (dbias_part) summed in float64.  Returns {name: (ratio, index)}."""
    dG = np.asarray(dG, F64)
    T, N, H4 = dG.shape
    s, sa = dG.sum((0, 1)), np.abs(dG).sum((0, 1))
    if slabs is not None:
        slabs = np.asarray(slabs, F64)
        out = {"dbias_part": worst_ratio(slabs.sum(0), s, g(T * N + 16) * sa + EPS32 * np.abs(s) + FLOOR)}
        dead = slabs[-(-N // 16):]
        out["dbias_part_zero_rows"] = (np.inf if (dead != 0).any() or not np.isfinite(slabs).all() else 0.0, -1)
        return out
    ref = np.asarray(old, F64) + s
    n_rb = -(-N // 16)
    return {"dbias": worst_ratio(got, ref, g(T * N + 16) * sa + n_rb * EPS32 * (np.abs(np.asarray(old, F64)) + sa) + FLOOR)}


# ------------------------------------------------------------------ cases: the smallest shape that reaches each kernel
# fam: gen (lstm_step_*_kernel), h64 (lstm_seq_*_h64), v5 (lstm_step_*_v5), pers (lstm_pers_*).  mode: precision of the
# recurrent product; st16: bf16 storage of h / dG; ndir entries with reverse flags `rev`; ldh2: both directions write
# columns of one [T, N, 2H] tensor; gld2: both directions' gates in one [T*N, 8H] tensor; shifts: step_shift per entry
# (driven through the _range entry points); bwd: arithmetic of the persistent backward launches ((): per-frame backward).
Case = collections.namedtuple("Case", "fam mode st16 H N T rev ldh2 gld2 shifts bwd note")


def _c(fam, mode, H, N, T, rev=(0,), st16=0, ldh2=0, gld2=0, shifts=None, bwd=(), note=""):
    return Case(fam, mode, st16, H, N, T, tuple(rev), ldh2, gld2, tuple(shifts or (0,) * len(rev)), tuple(bwd), note)


_V5_MODES = [(MODE_F32, 0), (MODE_F32X3, 0), (MODE_BF16, 0), (MODE_BF16, 1)]
CASES = [
    _c("gen", MODE_F32, 128, 17, 3, note="lstm_step_*_kernel<1>: two k-chunks, second row block with one live row"),
    _c("gen", MODE_F32, 192, 33, 4, rev=(0, 1), ldh2=1, note="three k-chunks (odd pipeline tail); n_j = 12: non-XCD block decode"),
    _c("gen", MODE_F32, 128, 1, 1, note="a single row, a single frame"),
    _c("h64", MODE_F32, 64, 20, 5, rev=(0, 1), ldh2=1, gld2=1, note="lstm_seq_*_h64<0>: gate_ld = 8H in one shared tensor"),
    _c("h64", MODE_F32, 64, 1, 1, note="lstm_seq_*_h64<0>: a single row, a single frame"),
] + [_c("h64", m, 64, N, 3, rev=(0, 1), ldh2=1, note=f"lstm_seq_*_h64<{m}, {r}>: {r}-row workgroups")
     for m in (MODE_F32X3, MODE_BF16) for N, r in ((5, 4), (130, 8), (258, 16))
] + [c for m, s in _V5_MODES for c in (
    _c("v5", m, 512, 17, 4, rev=(1,), st16=s, note="lstm_step_*_v5<1, ..>: 16-row tiles, reverse"),
    _c("v5", m, 1024, 97, 3, st16=s, note="lstm_step_*_v5<2, ..>: 32-row tiles, the fourth row block has one live row"),
    _c("v5", m, 512, 97, 3, rev=(0, 1), st16=s, ldh2=1, note="lstm_step_*_v5<2, ..>: 32-row tiles via ndir"),
    _c("v5", m, 1024, 97, 4, rev=(0, 0), st16=s, shifts=(0, 2), note="two stacked entries through the _range entry points (fp32: the 64-deep forward)"))
] + [
    _c("pers", MODE_BF16, 512, 40, 6, st16=1, bwd=(MODE_BF16,), note="lstm_pers_*_bf16<512, 1>"),
    _c("pers", MODE_BF16, 1024, 129, 5, bwd=(MODE_BF16,), note="lstm_pers_*_bf16<1024, 2>: 32-row workgroups"),
    _c("pers", MODE_F32X3, 1024, 17, 6, bwd=(MODE_F32X3, MODE_F32), note="lstm_pers_fwd_x3<1024>, bwd_x3k<1024>, bwd_f32<1024>"),
    _c("pers", MODE_F32X3, 512, 97, 7, rev=(1,), bwd=(MODE_F32X3, MODE_F32), note="lstm_pers_fwd_x3h<512> (8 units), bwd_x3<512, 0, 1> (16 rows), bwd_f32<512>"),
]
MODE_NAMES = {MODE_F32: "fp32", MODE_BF16: "bf16", MODE_F32X3: "fp32x3"}


def case_id(c):
    return (f"{c.fam}-{MODE_NAMES[c.mode]}{'-s16' if c.st16 else ''}-H{c.H}-N{c.N}-T{c.T}-"
            f"{'x'.join('r' if r else 'f' for r in c.rev)}{'-shift' if any(c.shifts) else ''}")


def make_entry(H, N, T, seed):
    """fp32 inputs of one entry (layer-direction): x [T, N, 4H] pre-activations uniform in +-2, W [4H, H] uniform in
    +-1/sqrt(H) with rows 2H+16 .. 2H+31 scaled x8, dh [T, N, H] uniform in +-1 with rows n % 5 == 2 exactly zero, old bias
    gradients db0 [2, 4H] uniform in +-2.  Unit classes by j % 16 (every 16-unit tile has each):
      3   f, i = +12, g = +-12 (sign by unit): the cell integrates to |c| ~ T, tanh(c) saturates;
      7   all four gates +-100: __expf overflows / underflows, the gates are exactly 0, 1 or +-1;
      11  all four gates scaled by 1e-4: the cancellation regime of gate_tanh.
    Row 0 has all-zero pre-activations at t = 0 and t = T - 1 (the first frame of either direction): gate_tanh(0) == 0."""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-2, 2, (T, N, 4, H))
    j = np.arange(H)
    k3, k7, k11 = j % 16 == 3, j % 16 == 7, j % 16 == 11
    x[:, :, 0, k3] = 12.0
    x[:, :, 1, k3] = 12.0
    x[:, :, 2, k3] = 12.0 * np.where((j[k3] // 16) % 2 == 0, 1.0, -1.0)
    x[:, :, :, k7] = 100.0 * rs.choice([-1.0, 1.0], (T, N, 4, int(k7.sum())))
    x[:, :, :, k11] *= 1e-4
    x[0, 0], x[T - 1, 0] = 0.0, 0.0
    W = rs.uniform(-1, 1, (4 * H, H)) / np.sqrt(H)
    W[2 * H + 16:2 * H + 32] *= 8.0
    dh = rs.uniform(-1, 1, (T, N, H))
    dh[:, np.arange(N) % 5 == 2] = 0.0
    d = {"x": x.reshape(T, N, 4 * H), "W": W, "dh": dh, "db0": rs.uniform(-2, 2, (2, 4 * H))}
    return {k: np.ascontiguousarray(v, dtype=F) for k, v in d.items()}


def make_inputs(case, seed=0):
    """One independent entry per direction / stacked entry of the case; the same for either storage of h / dG."""
    key = zlib.crc32(repr(tuple(case._replace(st16=0, note=""))).encode()) % 100000
    return [make_entry(case.H, case.N, case.T, 1000003 * seed + 17 * key + e) for e in range(len(case.rev))]


def stored_bf16_check(v16, v32, tol32):
    """A bf16-stored h or dG against the same case run with fp32 storage (in the bf16 mode both runs feed the next frame
    the same rounded operand): 2^-8 relative (BF16_REL) plus the fp32 bound of that element.  (ratio, flat index)."""
    v32 = np.asarray(v32, F64)
    return worst_ratio(v16, v32, BF16_REL * (np.abs(v32) + tol32) + tol32)


# ------------------------------------------------------------------ the kernels' statements in numpy float32
def gate_sigmoid_f32(x):
    with np.errstate(over="ignore", under="ignore"):
        return F(1) / (F(1) + np.exp(-np.asarray(x, F)))


def gate_tanh_f32(x):
    with np.errstate(over="ignore", under="ignore"):
        return F(1) - F(2) * (F(1) / (np.exp(F(2) * np.asarray(x, F)) + F(1)))


def fwd_f32(x, W, h_prev, c_prev, mode, fma, product=None):
    """One forward frame as the kernels state it, fp32: sequential products of the mode's operands, gate functions as in
    csrc/common.h, the epilogue with or without fused multiply-add.  `product`: another recurrent product (mutations)."""
    x = np.asarray(x, F)
    H = x.shape[1] // 4
    if h_prev is None:
        a, c_prev = x, np.zeros((x.shape[0], H), F)
    else:
        a = (product or seq_dot)(operand(h_prev, mode), operand(W, mode).T, x)
    i, f, o = gate_sigmoid_f32(a[:, :H]), gate_sigmoid_f32(a[:, H:2 * H]), gate_sigmoid_f32(a[:, 3 * H:])
    gg = gate_tanh_f32(a[:, 2 * H:3 * H])
    c = _fma(f, c_prev, i * gg) if fma else f * c_prev + i * gg
    return np.concatenate([i, f, gg, o], 1), c, o * gate_tanh_f32(c)


def bwd_f32(dh_out, W, dG_next, gates, c, c_prev, dcar, mode, fma):
    """One backward frame, fp32: (dgates, dcar')."""
    dh_out, c = np.asarray(dh_out, F), np.asarray(c, F)
    H = c.shape[1]
    dh = dh_out if dG_next is None else seq_dot(operand(dG_next, mode), operand(W, mode), dh_out)
    c_prev = np.zeros_like(c) if c_prev is None else np.asarray(c_prev, F)
    i, f, gg, o = (np.asarray(gates[:, q * H:(q + 1) * H], F) for q in range(4))
    tc = gate_tanh_f32(c)
    if fma:
        dc = _fma(dh * o, _fma(-tc, tc, F(1)), dcar)
        eg = _fma(-gg, gg, F(1))
    else:
        dc = np.asarray(dcar, F) + dh * o * (F(1) - tc * tc)
        eg = F(1) - gg * gg
    dG = np.concatenate([dc * gg * i * (F(1) - i), dc * c_prev * f * (F(1) - f), dc * i * eg, dh * tc * o * (F(1) - o)], 1)
    return dG, dc * f


def run_f32(e, reverse, mode, fma, h_bf16=False, g_bf16=False, product=None):
    """A whole direction on the fp32 restatement, free-running like a device: the `dev` dictionary of check_dir, with
    dc_steps."""
    x, W, dh = e["x"], e["W"], e["dh"]
    T, N, H = x.shape[0], x.shape[1], x.shape[2] // 4
    o = order(T, reverse)
    dev = {"gates": np.zeros((T, N, 4 * H), F), "c": np.zeros((T, N, H), F), "h": np.zeros((T, N, H), F),
           "dG": np.zeros((T, N, 4 * H), F)}
    for s, t in enumerate(o):
        tp = o[s - 1] if s else None
        gt, c, h = fwd_f32(x[t], W, None if tp is None else dev["h"][tp], None if tp is None else dev["c"][tp], mode, fma, product)
        dev["gates"][t], dev["c"][t], dev["h"][t] = gt, c, bf16(h) if h_bf16 else h
    dcar, steps = np.zeros((N, H), F), []
    for s in range(T - 1, -1, -1):
        t, tp, tn = o[s], (o[s - 1] if s else None), (o[s + 1] if s + 1 < T else None)
        dG, dcar = bwd_f32(dh[t], W, None if tn is None else dev["dG"][tn], dev["gates"][t], dev["c"][t],
                           None if tp is None else dev["c"][tp], dcar, mode, fma)
        dev["dG"][t] = bf16(dG) if g_bf16 else dG
        steps.append(dcar.copy())
    dev["dc"] = dcar
    return dev, steps
