"""float64 reference of the audio kernels of csrc/frontend.hip, entry point by entry point, as include/dvae_hip.h documents
them; what each launch may lose against it; the named input cases of tests/test_audio_ref.py (CPU) and
tests/test_hip_audio.py (MI355X).  numpy only.

Notation: eps32 = 2^-24, g(k) = k eps32 / (1 - k eps32) (k roundings compounded), FLOOR = 2^-126.  Device code is compiled
with contraction on: a * b + c may or may not be one fused operation, so every bound counts the roundings of the UNFUSED
form (fusing only removes one).  Every bound is a count of roundings times a sum of absolute values of what the launch
read, never a fraction of a maximum.

Device functions (scripts/probes/mathf_sweep.hip on the MI355X).  Worst |f32 result - float64| in
units of eps32 |float64 value| ("rel"; sincosf: in units of eps32, "abs", |value| <= 1), its argument, and the constant
used here = twice that (the sweep is a sample):
    log10f   [1e-5, 1e4] + the floats around 1     3.6173  at 0.00383908814
    logf     [1e-10, 1e8] + the floats around 1    3.1618  at 1.09220345e-07
    exp10f   [-4.2, 0.8]                           1.3934  at -0.884286702
    sincosf  [-64, 64]                             1.1740  at -3.90477395   (rel 2.0282 at -48.4415131, not used)
    sqrtf    every float of [1, 4)                 1.0000  (correctly rounded as far as the sweep sees)
    a / b    2^25 full-significand pairs           0.9999  (likewise)

Two input classes.  E: small integers and powers of two, every product, sum and quotient exact in fp32: the result must
match BIT FOR BIT whether or not the compiler fuses; a lost, doubled or misplaced term changes the integer.  R: full
significands with the edges mixed in, held to the bounds below at every element.

Bit for bit, no bound
    stft_frames / _seg      fl32(wav * win) inside [0, n), +0 outside: one product per element.
    gl_init, phase NULL     (mag | +0).
    gl_phase, |a| = 0       (mag | +0), also where rebuilt - alpha prev cancels exactly.
    mel_db_normalize        the clips at 0 and 1 (where the float64 value is beyond the clip by more than the bound) and the
                            floor (every input <= min_level gives the bits the input min_level gives).
    ola_gather              +0 outside [0, n) (mode 0), in the gaps (mode 1) and where the window envelope e <= 1e-20.
    resample_batch          +0 on n_valid <= t < n_out; class E.
    log_power               +0 in bins nb..nbp; one value below the floor.
    voicing_compact         feats: a copy; class E: peak, voiced, count.
    dtw_batch               class E: cost, length;  dtw_batch_f0: cost and length are dtw_batch's bits.
    the host tables         gl_segment_table, resample_segment_table, resample_lds_floats.

Bounded (|got - ref| <= tol, element by element; SQ, DV, LG10, LG, X10, SC the constants above)
    stft_magnitude   s = re^2 + im^2 carries <= 2 roundings (a product and the sum; fused: 1), sqrt halves them:
                     tol = (half(2) + SQ eps32 (1 + g(2))) |ref|, half(k) = g(k) (1 + g(k)) / 2.
    mel_db_normalize l = log10f(max(x, min_level)), db = 20 l - ref (2 roundings), q = (db - min_db) / -min_db:
                     tol = [ (g(LG10 + 1) |20 log10 v| + eps32 |db| + eps32 |db - min_db|) / |min_db| + g(DV) |q| ] (1 + g(8)),
                     carried through the clip (1-Lipschitz).
    mel_denormalize  db = c * -min_db + min_db + ref_db (3 roundings, on |t1|, |t2|, |t3|), a = db * 0.05f (1 rounding):
                     da = (0.05 eps32 (|t1| + |t2| + |t3|) + eps32 |a|) (1 + g(8));  tol = 10^a (expm1(ln10 da) + X10 eps32 (1 + ..)).
    gl_init          re = s cos(p): tol = SC eps32 |s| (1 + eps32) + eps32 |ref|  (sin likewise).
    gl_phase         a = reb - alpha prev: d = eps32 (|alpha prev| + |a|) per component; |a|^2 <= 2 roundings, sqrt, one
                     division, one product: tol = |s| (g(2 + SQ + DV) |a_re| / |a| + 2 |d| / |a|) where |d| < |a| / 4, nothing is
                     held (tol = +inf) where the cancellation leaves less.
    ola_gather       k = the frames that overlap the sample: s = sum w y and e = sum w^2 are k-term dot products,
                     |ds| <= g(k) sum |w y|, |de| <= g(k) e; norm: tol = (g(k) sum|w y| / e + (g(k) + g(DV)) |s / e|) (1 + g(k + 4));
                     mode 0 multiplies by |w| and adds eps32 |result|.
    resample_batch   an fp32 fma chain in tap order over the fp32 weights: tol = g(taps) sum |w x| + FLOOR.
    log_power        p: g(2) p.   log: g(LG) |ln p| + g(2) (1 + g(2)) above the floor.
    voicing_compact  peak = max(r gain) / r0: tol = g(1 + DV) |peak|; the flags wherever the float64 margins
                     |r0 - rel_min max r0| > eps32 rel_min max r0 and |peak - peak_min| > tol hold.
    dtw_batch        u = 2^-53.  A cell's distance (24 float64 fma and a square root against numpy's 24 products, a pairwise
                     sum and a square root) differs by at most 28 u d; the addition d + min(..) by u D on either side; min is
                     1-Lipschitz, so B(i,j) = 28 u d + 2 u D(i,j) + max over the predecessors of B bounds |D - D_ref| at every
                     cell (computed by the same recursion).  cost: B at the corner, which is <= (28 + 2 length) u cost along
                     the path.  length: equal wherever every cell of the reference's path chose its predecessor by a margin
                     above 2 max B(predecessors).  sse: fp32 running sum of fp32-rounded non-negative terms along the path,
                     tol = g(length + 1) sse.
"""
import numpy as np

import bn_ref as B

EPS32, EPS64, FLOOR, g, worst_ratio = B.EPS32, B.EPS64, B.FLOOR, B.g, B.worst_ratio
F64, F32 = np.float64, np.float32

# measured on the MI355X by scripts/probes/mathf_sweep.hip (worst, and where); the bound constants are twice that
LOG10F_MEASURED, LOG10F_AT = 3.6173, 0.00383908814
LOGF_MEASURED, LOGF_AT = 3.1618, 1.09220345e-07
EXP10F_MEASURED, EXP10F_AT = 1.3934, -0.884286702
SINCOSF_MEASURED, SINCOSF_AT = 1.1740, -3.90477395
SQRTF_MEASURED, SQRTF_AT = 1.0000, 1.00000012
DIVF_MEASURED, DIVF_AT = 0.9999, (2467.47998, 616.866943)
LG10, LG, X10, SC = 2 * LOG10F_MEASURED, 2 * LOGF_MEASURED, 2 * EXP10F_MEASURED, 2 * SINCOSF_MEASURED
SQ, DV = 2 * SQRTF_MEASURED, 2 * DIVF_MEASURED
EXP10F_DOMAIN = (-4.2, 0.8)            # what the sweep covered; mel_denormalize is held to its bound inside it only

MCD_DIM = 24
RS_TILE, DTW_THREADS, VC_THREADS = 256, 256, 256


def half(k):
    return 0.5 * g(k) * (1.0 + g(k))


def f32(a):
    return np.ascontiguousarray(a, F32)


def nextf(a, up):
    return np.nextafter(F32(a), F32(np.inf if up else -np.inf))


# ------------------------------------------------------------------ segment tables (host entry points)
def gl_segment_table(frames, fsize, hop):
    """dvae_gl_segment_table: [nseg, 4] int64 {row0, M, sample0, n}, None where it refuses"""
    if len(frames) < 1 or fsize < 4 or fsize % 4 or hop < 4 or hop % 4 or hop > fsize or fsize % hop:
        return None
    t, row0, s0 = [], 0, 0
    for M in frames:
        if M < fsize // hop:
            return None
        n = (M - fsize // hop + 1) * hop
        t.append([row0, M, s0, n])
        row0, s0 = row0 + M, s0 + n
    return np.array(t, np.int64)


def seg_table(frames, ns, gap=0):
    """a hand-built table of the same layout: utterance s has frames[s] rows and ns[s] samples, `gap` samples apart"""
    t, row0, s0 = [], 0, 0
    for M, n in zip(frames, ns):
        t.append([row0, M, s0, n])
        row0, s0 = row0 + M, s0 + n + gap
    return np.array(t, np.int64)


# ------------------------------------------------------------------ stft_frames
def frames_ref(wav, win, segs, rows, fsize, hop, left, dtype=F32, win_shift=0):
    """frames[r][k] = fl32(win[k] wav[sample0 + (r - row0) hop + k - left]) inside [0, n), +0 outside.  win_shift: the
    seeded mistake (window index off by one)."""
    wav, win = np.asarray(wav, dtype), np.asarray(win, dtype)
    out = np.zeros((rows, fsize), dtype)
    k = np.arange(fsize)
    for row0, M, s0, n in np.asarray(segs, np.int64):
        for m in range(int(M)):
            if row0 + m >= rows:
                break
            i = m * hop + k - left
            ok = (i >= 0) & (i < n)
            out[row0 + m, ok] = wav[s0 + i[ok]] * win[(k[ok] + win_shift) % fsize]
    return out


# ------------------------------------------------------------------ stft_magnitude
def magnitude_bounds(reim, nbp):
    r = np.asarray(reim, F64)
    ref = np.sqrt(r[:, :nbp] ** 2 + r[:, nbp:2 * nbp] ** 2)
    return ref, (half(2) + SQ * EPS32 * (1 + g(2))) * ref + FLOOR


def magnitude_f32(reim, nbp, fma, push=0.0):
    """the kernel's order in fp32; fma: the square-sum fused; push: sqrtf wrong by +-(SQ - 1) roundings before its own"""
    re, im = f32(reim)[:, :nbp], f32(reim)[:, nbp:2 * nbp]
    if fma:
        s = (re.astype(F64) ** 2 + (im * im).astype(F64)).astype(F32)
    else:
        s = re * re + im * im
    return (np.sqrt(s.astype(F64)) * (1 + push * (SQ - 1) * EPS32)).astype(F32)


# ------------------------------------------------------------------ mel_db_normalize / mel_denormalize
def db_normalize_bounds(mel, min_level, ref_db, min_db, log=np.log10):
    """mel [M, C] -> (ref [C, M], tol [C, M], q before the clip).  log: the seeded mistake takes np.log"""
    min_level, ref_db, min_db = F64(F32(min_level)), F64(F32(ref_db)), F64(F32(min_db))
    v = np.maximum(np.asarray(mel, F64), min_level).T
    l20 = 20.0 * log(v)
    db = l20 - ref_db
    q = (db - min_db) / -min_db
    b = ((g(LG10 + 1) * np.abs(l20) + EPS32 * np.abs(db) + EPS32 * np.abs(db - min_db)) / abs(min_db) + g(DV) * np.abs(q)) \
        * (1 + g(8)) + FLOOR
    tol = np.where((q < -b) | (q > 1 + b), FLOOR, b)           # beyond a clip by more than the bound: the clip's bits
    return np.clip(q, 0.0, 1.0), tol, q


def db_normalize_f32(mel, min_level, ref_db, min_db, fma, push=0.0):
    v = np.maximum(f32(mel), F32(min_level)).T
    l = (np.log10(v.astype(F64)) * (1 + push * (LG10 - 1) * EPS32)).astype(F32)
    if fma:
        db = (20.0 * l.astype(F64) - F64(F32(ref_db))).astype(F32)
    else:
        db = F32(20) * l - F32(ref_db)
    q = (db - F32(min_db)) / -F32(min_db)
    return np.clip(q, F32(0), F32(1))


def denormalize_bounds(mel, ref_db, min_db):
    """mel [C, L] -> (amp [L, C], tol); +inf where the exponent leaves the swept domain of exp10f"""
    ref_db, min_db = F64(F32(ref_db)), F64(F32(min_db))
    c = np.clip(np.asarray(mel, F64), 0.0, 1.0).T
    t1 = c * -min_db
    t2 = t1 + min_db
    t3 = t2 + ref_db
    a = t3 * F64(F32(0.05))
    da = (F64(F32(0.05)) * EPS32 * (np.abs(t1) + np.abs(t2) + np.abs(t3)) + EPS32 * np.abs(a)) * (1 + g(8))
    ref = 10.0 ** a
    tol = ref * (np.expm1(np.log(10.0) * da) + X10 * EPS32 * (1 + np.log(10.0) * da) * (1 + g(2))) + FLOOR
    inside = (a >= EXP10F_DOMAIN[0] - 1e-6) & (a <= EXP10F_DOMAIN[1] + 1e-6)
    return ref, np.where(inside, tol, np.inf)


def denormalize_f32(mel, ref_db, min_db, fma, push=0.0):
    c = np.clip(f32(mel), F32(0), F32(1)).T
    if fma:
        t2 = (c.astype(F64) * -F64(F32(min_db)) + F64(F32(min_db))).astype(F32)
    else:
        t2 = c * -F32(min_db) + F32(min_db)
    a = (t2 + F32(ref_db)) * F32(0.05)
    return (10.0 ** a.astype(F64) * (1 + push * (X10 - 1) * EPS32)).astype(F32)


# ------------------------------------------------------------------ gl_init / gl_phase
def gl_init_bounds(mag, phase, swap=False):
    """(reim [rows, 2 nbp], tol); phase None: exact (tol 0).  swap: the seeded mistake (imaginary block first)"""
    s = np.asarray(mag, F64)
    if phase is None:
        re, im, tr, ti = s, np.zeros_like(s), np.full_like(s, FLOOR), np.full_like(s, FLOOR)
    else:
        p = np.asarray(phase, F64)
        re, im = s * np.cos(p), s * np.sin(p)
        tr = SC * EPS32 * np.abs(s) * (1 + EPS32) + EPS32 * np.abs(re) + FLOOR
        ti = SC * EPS32 * np.abs(s) * (1 + EPS32) + EPS32 * np.abs(im) + FLOOR
    if swap:
        re, im = im, re
    return np.concatenate([re, im], 1), np.concatenate([tr, ti], 1)


def gl_alpha(momentum):
    """what the entry point hands the kernel: fp32 momentum / (1 + momentum), both operations rounded"""
    m = F32(momentum)
    return F32(m / F32(F32(1) + m))


def gl_phase_bounds(reb, prev, mag, nbp, momentum, zero_branch=None):
    """(reim, tol, exact): `exact` marks the elements whose a is exactly 0 in float64 AND in any fp32 evaluation (both
    components: the operand is 0 or the product alpha prev is exact and equals rebuilt) -> (mag, +0) bit for bit.
    zero_branch: the seeded mistake's value of the |a| = 0 branch"""
    al = F64(gl_alpha(momentum))
    R, s = np.asarray(reb, F64), np.asarray(mag, F64)
    Pv = np.zeros_like(R) if prev is None else np.asarray(prev, F64)
    a = R - al * Pv
    d = EPS32 * (np.abs(al * Pv) + np.abs(a)) if prev is not None else np.zeros_like(a)
    are, aim, dre, dim_ = a[:, :nbp], a[:, nbp:], d[:, :nbp], d[:, nbp:]
    na, nd = np.hypot(are, aim), np.hypot(dre, dim_)
    prod_exact = (al * Pv).astype(F32).astype(F64) == al * Pv
    zero = (na == 0) & prod_exact[:, :nbp] & prod_exact[:, nbp:]
    with np.errstate(divide="ignore", invalid="ignore"):
        re = np.where(na > 0, s * are / na, s if zero_branch is None else zero_branch)
        im = np.where(na > 0, s * aim / na, 0.0)
        k = g(2 + SQ + DV)
        tr = np.abs(s) * (k * np.abs(are) + 2 * nd) / na + FLOOR
        ti = np.abs(s) * (k * np.abs(aim) + 2 * nd) / na + FLOOR
    held = nd < na / 4
    tr, ti = np.where(held, tr, np.inf), np.where(held, ti, np.inf)
    tr, ti = np.where(zero, FLOOR, tr), np.where(zero, FLOOR, ti)
    return np.concatenate([re, im], 1), np.concatenate([tr, ti], 1), np.concatenate([zero, zero], 1)


def gl_phase_f32(reb, prev, mag, nbp, momentum, fma):
    al, R, s = gl_alpha(momentum), f32(reb), f32(mag)
    if prev is None:
        a = R
    elif fma:
        a = (R.astype(F64) - F64(al) * f32(prev).astype(F64)).astype(F32)
    else:
        a = R - al * f32(prev)
    are, aim = a[:, :nbp], a[:, nbp:]
    if fma:
        a2 = (are.astype(F64) ** 2 + (aim * aim).astype(F64)).astype(F32)
    else:
        a2 = are * are + aim * aim
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = s / np.sqrt(a2)
        re, im = np.where(a2 > 0, are * inv, s), np.where(a2 > 0, aim * inv, F32(0))
    return np.concatenate([re, im], 1).astype(F32)


# ------------------------------------------------------------------ ola_gather
def ola_signal(y, win, M, P, fsize, hop, norm, m_lo_plus=1):
    """float64 s, tol and overlap count of padded position P of one utterance's frames y [M, fsize] (csrc ola4);
    m_lo_plus = 0: the seeded mistake (one frame too many at the lower end; outside the window it reads zeros here)"""
    m_hi = min(M - 1, P // hop)
    m_lo = (P - fsize) // hop + m_lo_plus if P >= fsize else 0
    s = e = sa = 0.0
    k = 0
    for m in range(m_lo, m_hi + 1):
        q = P - m * hop
        w = float(win[q]) if q < fsize else 1.0
        v = float(y[m, q]) if q < fsize else float(y[min(m + 1, M - 1), q - fsize])
        s, e, sa, k = s + w * v, e + w * w, sa + abs(w * v), k + 1
    if not norm:
        return s, g(k) * sa, k
    if not e > 1e-20:
        return 0.0, 0.0, k                                       # the envelope branch: +0 exactly
    return s / e, (g(k) * sa / e + (g(k) + g(DV)) * abs(s / e)) * (1 + g(k + 4)), k


def ola_bounds(y, win, segs, rows, out_len, fsize, hop, mode, norm, m_lo_plus=1, skip_norm_div=False):
    """(ref, tol) of dvae_ola_gather: mode 0 [rows, fsize], mode 1 [out_len].  skip_norm_div: the seeded mistake"""
    y, win = np.asarray(y, F64), np.asarray(win, F64)
    left = fsize - hop
    ref = np.zeros((rows, fsize) if mode == 0 else (out_len,))
    tol = np.full_like(ref, FLOOR)
    for row0, M, s0, n in np.asarray(segs, np.int64):
        yy = y[row0:row0 + M]
        sig = [ola_signal(yy, win, int(M), t + left, fsize, hop, norm and not skip_norm_div, m_lo_plus) for t in range(int(n))]
        for t, (s, b, _) in enumerate(sig):
            if mode == 1:
                ref[s0 + t], tol[s0 + t] = s, b + FLOOR
            else:
                for m in range(int(M)):
                    k = t - m * hop + left
                    if 0 <= k < fsize:
                        ref[row0 + m, k] = s * win[k]
                        tol[row0 + m, k] = b * abs(win[k]) + EPS32 * abs(s * win[k]) + FLOOR
    return ref, tol


def ola_f32(y, win, segs, rows, out_len, fsize, hop, mode, norm, fma):
    """the kernel's order in fp32, the products fused into the running sums or not"""
    y, win = f32(y), f32(win)
    left = fsize - hop
    out = np.zeros((rows, fsize) if mode == 0 else (out_len,), F32)

    def mac(acc, a, b):
        return F32(F64(acc) + F64(a) * F64(b)) if fma else F32(acc + F32(a * b))
    for row0, M, s0, n in np.asarray(segs, np.int64):
        for t in range(int(n)):
            P = t + left
            s = e = F32(0)
            for m in range((P - fsize) // hop + 1 if P >= fsize else 0, min(int(M) - 1, P // hop) + 1):
                q = P - m * hop
                s, e = mac(s, win[q], y[row0 + m, q]), mac(e, win[q], win[q])
            if norm:
                s = F32(s / e) if e > F32(1e-20) else F32(0)
            if mode == 1:
                out[s0 + t] = s
            else:
                for m in range(int(M)):
                    k = t - m * hop + left
                    if 0 <= k < fsize:
                        out[row0 + m, k] = s * win[k]
    return out


# ------------------------------------------------------------------ resampling
def resample_segment_table(n_in, filt, filters, tile, max_tiles=1 << 40, ceil_valid=False):
    """dvae_resample_segment_table: (table [nseg, 6], tiles [ntiles, 2]) or None where it refuses.  ceil_valid: the
    seeded mistake (n_valid taken as the ceiling)"""
    table, tiles, in0, out0 = [], [], 0, 0
    if len(n_in) < 1 or len(filters) < 1 or tile < 1:
        return None
    for s, (n, f) in enumerate(zip(n_in, filt)):
        if f < 0 or f >= len(filters) or n < 1:
            return None
        P, Q = int(filters[f][0]), int(filters[f][1])
        if P < 1 or Q < 1 or n > (1 << 40) // max(P, Q):
            return None
        n_out = -(-n * P // Q)
        n_valid = n_out if ceil_valid else n * P // Q
        if n_valid < 1:
            return None
        table.append([in0, n, out0, n_out, n_valid, f])
        for t0 in range(0, n_out, tile):
            if len(tiles) >= max_tiles:
                return None
            tiles.append([s, t0])
        in0, out0 = in0 + (n + 3) // 4 * 4, out0 + (n_out + 3) // 4 * 4
    return np.array(table, np.int64), np.array(tiles, np.int64)


def resample_lds_floats(P, Q, taps):
    if P < 1 or Q < 1 or taps < 1:
        return None
    span = ((RS_TILE - 1) * Q + P - 1) // P + 1 + taps + 4
    cap = (span + 3) // 4 * 4
    return None if cap * 4 > 64 * 1024 else cap


def resample_bounds(x, table, filters, weights, drop_tap=None):
    """(y [packed outputs] float64, tol, sentinel-free).  x: the packed inputs; weights fp32.  drop_tap: seeded mistake"""
    x, w = np.asarray(x, F64), np.asarray(weights, F64)
    total = int(table[-1][2] + (table[-1][3] + 3) // 4 * 4)
    y, tol = np.zeros(total), np.full(total, FLOOR)
    written = np.zeros(total, bool)
    for in0, n_in, out0, n_out, n_valid, f in np.asarray(table, np.int64):
        P, Q, taps, base, woff, _ = [int(v) for v in filters[f]]
        t = np.arange(n_valid)
        m = t * Q // P
        ph = t * Q - m * P
        idx = (m - base)[:, None] + np.arange(taps)[None, :]
        ok = (idx >= 0) & (idx < n_in)
        xs = np.where(ok, x[in0 + np.clip(idx, 0, n_in - 1)], 0.0)
        ws = w[woff + ph[:, None] * taps + np.arange(taps)[None, :]]
        if drop_tap is not None:
            ws = ws.copy()
            ws[:, drop_tap % taps] = 0.0
        y[out0:out0 + n_valid] = (ws * xs).sum(1)
        tol[out0:out0 + n_valid] = g(taps) * np.abs(ws * xs).sum(1) + FLOOR
        written[out0:out0 + n_out] = True
    return y, tol, written


def resample_f32(x, table, filters, weights, fma=True):
    """the kernel's fp32 chain in tap order (fma: one rounding per tap, as written; else two)"""
    x, w = f32(x), f32(weights)
    total = int(table[-1][2] + (table[-1][3] + 3) // 4 * 4)
    y = np.zeros(total, F32)
    for in0, n_in, out0, n_out, n_valid, f in np.asarray(table, np.int64):
        P, Q, taps, base, woff, _ = [int(v) for v in filters[f]]
        t = np.arange(n_valid)
        m = t * Q // P
        ph = t * Q - m * P
        acc = np.zeros(n_valid, F32)
        for c in range(taps):
            i = m - base + c
            xv = np.where((i >= 0) & (i < n_in), x[in0 + np.clip(i, 0, n_in - 1)], F32(0))
            wv = w[woff + ph * taps + c]
            acc = (acc.astype(F64) + wv.astype(F64) * xv.astype(F64)).astype(F32) if fma else acc + wv * xv
        y[out0:out0 + n_valid] = acc
    return y


def resample_geometry(table, filters, lds_floats):
    """what each tile of the launch reaches: (g0 negative, unaligned g0, scalar edge loads, partial tile, zero-fill tail)"""
    seen = dict(g0_negative=0, unaligned=0, edge_loads=0, partial=0, tail=0, tiles=0, worst_j1=0)
    for in0, n_in, out0, n_out, n_valid, f in np.asarray(table, np.int64):
        P, Q, taps, base, woff, _ = [int(v) for v in filters[f]]
        for t0 in range(0, int(n_out), RS_TILE):
            seen["tiles"] += 1
            t_end = min(t0 + RS_TILE, n_valid)
            seen["tail"] += int(n_valid < min(t0 + RS_TILE, n_out))
            if t0 >= t_end:
                continue
            lo, hi = t0 * Q // P - base, (t_end - 1) * Q // P - base + taps
            g0 = in0 + lo
            a0 = g0 & ~3
            seen["g0_negative"] += int(g0 < 0)
            seen["unaligned"] += int(g0 != a0)
            seen["edge_loads"] += int(a0 < in0 or a0 + (hi - lo) + (g0 - a0) > in0 + n_in)
            seen["partial"] += int(t_end - t0 < RS_TILE)
            seen["worst_j1"] = max(seen["worst_j1"], (hi - lo) + (g0 - a0))
    assert seen["worst_j1"] <= lds_floats, "the named case itself would trip the kernel's NaN sentinel"
    return seen


# ------------------------------------------------------------------ log_power
def log_power_bounds(reim, nb, nbp, floor):
    """(power, tol_p, log, tol_l, below): below marks the bins certainly under the floor (one value, bit for bit)"""
    r = np.asarray(reim, F64)
    fl = F64(F32(floor))
    p = r[:, :nbp] ** 2 + r[:, nbp:2 * nbp] ** 2
    p[:, nb:] = 0.0
    tp = g(2) * p + FLOOR
    l = np.log(np.maximum(p, fl))
    rel = g(2) * (1 + g(2))
    tl = g(LG) * np.abs(l) + np.where(p * (1 + rel) > fl, rel, 0.0) + FLOOR
    tp[:, nb:], tl[:, nb:], l[:, nb:] = FLOOR, FLOOR, 0.0
    below = p * (1 + rel) <= fl
    below[:, nb:] = False
    return p, tp, l, tl, below


def log_power_f32(reim, nb, nbp, floor, fma, push=0.0):
    re, im = f32(reim)[:, :nbp], f32(reim)[:, nbp:2 * nbp]
    p = (re.astype(F64) ** 2 + (im * im).astype(F64)).astype(F32) if fma else re * re + im * im
    l = (np.log(np.maximum(p, F32(floor)).astype(F64)) * (1 + push * (LG - 1) * EPS32)).astype(F32)
    p[:, nb:], l[:, nb:] = 0, 0
    return p, l


# ------------------------------------------------------------------ voicing_compact
def voicing_bounds(r, nlag, gain, mc, segs, peak_min, rel_min, strict=False):
    """float64 restatement over a packed batch: dict(peak, tol_peak, voiced, decided (the flags the bounds decide), feats
    [rows, 24] fp32 (NaN where nothing is written), count).  strict: the seeded mistake (> for >=)"""
    r64, gn = np.asarray(r, F64), np.asarray(gain, F64)
    rows = r64.shape[0]
    pm, rm = F64(F32(peak_min)), F64(F32(rel_min))
    peak, tolp = np.zeros(rows), np.zeros(rows)
    voiced, decided = np.zeros(rows, np.int32), np.ones(rows, bool)
    feats = np.full((rows, MCD_DIM), np.nan, F32)
    count = []
    for row0, M, _, _ in np.asarray(segs, np.int64):
        rr = r64[row0:row0 + M]
        r0 = rr[:, 0]
        thr = rm * (r0.max() if M else 0.0)
        q = np.maximum((rr[:, 1:nlag + 1] * gn[None, 1:nlag + 1]).max(1), 0.0)
        p = np.where(r0 > 0, q / np.where(r0 > 0, r0, 1.0), 0.0)
        tp = g(1 + DV) * np.abs(p)
        v = (r0 > 0) & (r0 >= thr) & ((p > pm) if strict else (p >= pm))
        dec = ((np.abs(r0 - thr) > EPS32 * thr) | (r0 == thr)) & ((np.abs(p - pm) > tp) | (p == pm)) | (r0 <= 0)
        peak[row0:row0 + M], tolp[row0:row0 + M], voiced[row0:row0 + M], decided[row0:row0 + M] = p, tp + FLOOR, v, dec
        idx = np.nonzero(v)[0]
        feats[row0:row0 + len(idx)] = np.asarray(mc, F32)[row0 + idx, :MCD_DIM]
        count.append(len(idx))
    return dict(peak=peak, tol_peak=tolp, voiced=voiced, decided=decided, feats=feats, count=np.array(count, np.int32))


def voicing_e_case(M, nlag, pattern, seed, ldr=None, ldm=24):
    """class E inputs of one utterance: r(0) powers of two, r and gain powers of two / small integers, so r gain, the
    quotient by r(0) and rel_min max r(0) are exact.  peak_min = 1/2, rel_min = 2^-4, max r(0) = 16 (thr = 1).  Frames, by
    `pattern` ('all', 'none', 'alt', 'last_of_chunk', 'first_of_next', 'edges'), are voiced or fail ONE condition by the
    smallest amount: peak == 1/2 exactly (voiced), 1/2 - 2^-25 (not), r(0) == thr exactly (voiced), r(0) = thr / 2 (not),
    r(0) = 0 (not)."""
    rs = np.random.RandomState(seed)
    ldr = ldr or nlag + 1
    f = np.arange(M)
    want = {"all": np.ones(M, bool), "none": np.zeros(M, bool), "alt": f % 2 == 0, "last_of_chunk": f % 256 == 255,
            "first_of_next": (f % 256 == 0) & (f > 0), "edges": rs.rand(M) < 0.5}[pattern]
    r = np.full((M, ldr), np.nan, F32)
    gain = np.full(ldr, np.nan, F32)                            # column 0 of gain is never read: NaN
    gain[1:nlag + 1] = 2.0 ** np.random.RandomState(nlag).randint(-1, 2, nlag)     # by nlag alone: utterances of a batch share it
    kind = rs.randint(0, 5, M)                                  # how a frame passes / fails
    for i in range(M):
        r0 = F32(2.0 ** rs.randint(0, 4))                       # 1 .. 8: thr = 1 <= r0
        if want[i]:
            if kind[i] == 0:
                r0 = F32(1.0)                                   # r(0) == thr exactly
            top = F32(0.5) * r0 if kind[i] < 3 else r0          # peak == 1/2 exactly, or 1
        else:
            if kind[i] == 0:
                r0, top = F32(0.0), F32(4.0)
            elif kind[i] == 1:
                r0, top = F32(0.5), F32(0.5)                    # peak 1, r(0) = thr / 2
            else:
                top = F32(0.5) * r0 * F32(1 - 2.0 ** -24)       # peak = 1/2 - 2^-25: representable, one ulp below
        lag = rs.randint(1, nlag + 1)
        row = -np.abs(rs.randint(0, 3, nlag + 1)).astype(F32)   # the other lags: <= 0, below the peak
        row[lag] = top / gain[lag]
        row[0] = r0
        r[i, :nlag + 1] = row
    if M:
        r[rs.randint(0, M), 0] = 16.0                           # the utterance's loudest frame: thr = 1
        i = int(np.argmax(r[:, 0] == 16.0))
        lag = int(np.nanargmax(r[i, 1:nlag + 1] * gain[1:nlag + 1])) + 1
        r[i, lag] = (8.0 if want[i] else 4.0) / gain[lag]       # peak 1/2 (voiced) or 1/4
    mc = np.full((M, ldm), np.nan, F32)
    mc[:, :MCD_DIM] = rs.randint(-99, 100, (M, MCD_DIM))
    return r, gain, mc


def voicing_geometry(M):
    return dict(chunks=-(-M // VC_THREADS), partial_chunk=M % VC_THREADS != 0, partial_wave=M % 64 != 0)


# ------------------------------------------------------------------ DTW
def dist_matrix(x, y, dtype=F64):
    x, y = np.asarray(x, F32).astype(dtype), np.asarray(y, F32).astype(dtype)
    d = np.zeros((len(x), len(y)), dtype)
    for c in range(x.shape[1]):
        t = x[:, c][:, None] - y[:, c][None, :]
        d += t * t
    return np.sqrt(d).astype(F64)


def dtw_full(x, y, lx=None, ly=None, order=(0, 1, 2), dist_dtype=F64):
    """Exact DTW over the whole matrix, anti-diagonal by anti-diagonal: D(i,j) = d + min(D(i-1,j), D(i,j-1), D(i-1,j-1)), a
    tie to the first in that order.  -> dict(cost, length, sse, bound (B at the corner), margin_ok (every decision on the
    path is above 2 max B of its predecessors), min_margin, path_cells).  order: the seeded mistake permutes the preference
    ((2, 0, 1): diagonal first); dist_dtype float32: an fp32 dist_row."""
    N, M = len(x), len(y)
    if N == 0 or M == 0:
        return dict(cost=np.nan, length=0, sse=np.nan, bound=0.0, margin_ok=True, min_margin=np.inf)
    d = dist_matrix(x, y, dist_dtype)
    u = 2.0 ** -53
    D, Bd = np.full((N + 1, M + 1), np.inf), np.zeros((N + 1, M + 1))      # one row / column of +inf in front
    K, Mg = np.zeros((N, M), np.int8), np.full((N, M), np.inf)
    for dg in range(N + M - 1):
        i = np.arange(max(0, dg - M + 1), min(N - 1, dg) + 1)
        j = dg - i
        if dg == 0:
            D[1, 1], Bd[1, 1] = d[0, 0], 28 * u * d[0, 0]
            continue
        cand = np.stack([D[i, j + 1], D[i + 1, j], D[i, j]])              # (i-1, j), (i, j-1), (i-1, j-1)
        bnd = np.stack([Bd[i, j + 1], Bd[i + 1, j], Bd[i, j]])
        pref = cand[list(order)]
        k = np.asarray(order)[np.argmin(pref, axis=0)]
        cols = np.arange(len(i))
        best = cand[k, cols]
        srt = np.sort(cand, axis=0)
        K[i, j] = k
        with np.errstate(invalid="ignore"):
            Mg[i, j] = np.where(np.isfinite(srt[1]), srt[1] - srt[0], np.inf) - 2 * np.where(np.isfinite(cand), bnd, 0).max(0)
        D[i + 1, j + 1] = d[i, j] + best
        Bd[i + 1, j + 1] = 28 * u * d[i, j] + 2 * u * D[i + 1, j + 1] + np.where(np.isfinite(cand), bnd, 0).max(0)
    i, j, length, sse, mm = N - 1, M - 1, 1, 0.0, np.inf
    terms = []
    ties = dict(up_left=0, up_diag=0, left_diag=0, all3=0)
    names = {(1, 1, 0): "up_left", (1, 0, 1): "up_diag", (0, 1, 1): "left_diag", (1, 1, 1): "all3"}
    while True:
        if lx is not None:
            terms.append((F64(lx[i]) - F64(ly[j])) ** 2)
        if i == 0 and j == 0:
            break
        mm = min(mm, Mg[i, j])
        c = np.array([D[i, j + 1], D[i + 1, j], D[i, j]])
        key = names.get(tuple((c == c.min()).astype(int)))
        if key:
            ties[key] += 1
        i, j = (i - 1, j) if K[i, j] == 0 else ((i, j - 1) if K[i, j] == 1 else (i - 1, j - 1))
        length += 1
    sse = float(np.sum(terms)) if terms else np.nan
    return dict(cost=float(D[N, M]), length=length, sse=sse, bound=float(Bd[N, M]) + FLOOR, margin_ok=bool(mm > 0),
                min_margin=float(mm), ties=ties, tol_sse=g(length + 1) * sse + FLOOR if terms else 0.0)


def dtw_geometry(nx, ny):
    na = min(nx, ny)
    return dict(swap=nx > ny, slots=-(-na // DTW_THREADS), diagonals=nx + ny - 1)


def _rows(vals):
    """[n, 24] fp32 rows that differ in column 0 only: the distance of two rows is |difference| exactly"""
    a = np.zeros((len(vals), MCD_DIM), F32)
    a[:, 0] = vals
    a[:, 1:] = np.arange(1, MCD_DIM, dtype=F32)[None, :]
    return a


DTW_TIE_ORDERS = {"up_left": (1, 0, 2), "up_diag": (2, 0, 1), "left_diag": (0, 2, 1)}     # the preference that flips each pairing
DTW_TIE_SEEDS = {'up_left_3x4': 237, 'up_diag_3x4': 10, 'left_diag_3x4': 0, 'up_left_4x3': 667, 'up_diag_4x3': 2,
                 'left_diag_4x3': 0, 'mixed_257x258': 0, 'mixed_258x257': 0}


def dtw_e_cases():
    """name -> (x, y, expected length or None).  All distances are small integers: every D is exact, every tie is a tie on
    the device too.  'equal': every step ties three ways -> the documented order walks (i-1, j) first: length nx + ny - 1
    (a diagonal preference gives max(nx, ny)).  'up_left', 'up_diag', 'left_diag' at 3 x 4 and 4 x 3: sequences over
    {0, 1, 2} (seeds found by search) on whose path exactly that pairing of two predecessors ties, the third being larger,
    and the other preference for the pair gives another length.  'mixed' at 257 x 258 and 258 x 257: all three pairings tie
    on the path (thread slots 0 and 1 of the kernel), and each flipped preference gives another length."""
    out = {}
    for nx, ny in ((3, 4), (4, 3), (257, 258), (258, 257)):
        out[f"equal_{nx}x{ny}"] = (_rows(np.full(nx, 3.0)), _rows(np.full(ny, 3.0)), nx + ny - 1)
    for name, seed in DTW_TIE_SEEDS.items():
        nx, ny = [int(v) for v in name.rsplit("_", 1)[1].split("x")]
        rs = np.random.RandomState(seed)
        out[name] = (_rows(rs.randint(0, 3, nx)), _rows(rs.randint(0, 3, ny)), None)
    return out


# ------------------------------------------------------------------ named shapes (the GPU module walks all of them)
CASES = {
    # fsize, hop, left, n: left of 0 and of fsize - hop; n of 1, 3, 4, 5 and hop k +- 1
    "frames": [(8, 4, 0, 1), (8, 4, 4, 3), (8, 4, 4, 4), (8, 4, 0, 5), (16, 4, 12, 11), (16, 4, 12, 13), (16, 4, 0, 4),
               (12, 12, 0, 35), (12, 12, 0, 37), (12, 12, 0, 1), (16, 4, 12, 5)],
    "frames_seg": [(8, 4, 4, (1, 5, 37)), (16, 4, 12, (1, 5, 37)), (12, 12, 0, (1, 5, 37))],
    "rows_nbp": [(1, 1), (3, 5), (2, 516), (257, 4)],
    "transpose": [(1, 1), (31, 33), (32, 32), (33, 31), (65, 80)],
    "ola": [(8, 4), (16, 4), (8, 8), (24, 8), (20, 8)],
    "log_power": [(1, 1, 4), (3, 5, 8), (2, 513, 516), (65, 3, 4)],
    "voicing_M": [1, 63, 64, 65, 255, 256, 257, 513],
    "voicing_nlag": [1, 63, 64, 65, 206],
    "dtw_r": [(1, 1), (1, 5), (5, 1), (2, 2), (255, 257), (256, 256), (257, 255), (257, 300), (513, 520), (520, 513)],
    # taps, P, Q
    "resample_filters": [(4, 1, 3), (1, 1, 1), (9, 2, 3), (4, 3, 2), (9, 160, 441), (1, 2, 3), (9, 1, 1)],
    "resample_n_valid": [1, 2, 255, 256, 257, 513],
}


def rfull(rs, shape, lo=-8, hi=8):
    """class R: full significands over 2^lo .. 2^hi of either sign"""
    return ((1.0 + rs.rand(*shape)) * 2.0 ** rs.randint(lo, hi, shape) * rs.choice([-1.0, 1.0], shape)).astype(F32)


def frames_count(n, fsize, hop, left):
    """rows whose frame touches the signal at all, + 1 (an all-padding row: zeros)"""
    return max(1, -(-(n + left) // hop)) + 1


def db_edge_values(rs, M, C, min_level, ref_db, min_db):
    """class R input of mel_db_normalize: log-uniform values with the floor, either clip and one ulp to each side mixed in"""
    x = (10.0 ** rs.uniform(np.log10(min_level) - 1, 1.2, (M, C))).astype(F32)
    lo, hi = F32(10.0 ** ((min_db + ref_db) / 20.0)), F32(10.0 ** (ref_db / 20.0))
    edges = []
    for v in (F32(min_level), lo, hi):
        edges += [v, nextf(v, True), nextf(v, False)]
    flat = x.reshape(-1)
    pos = rs.permutation(flat.size)[:len(edges)]
    flat[pos] = np.array(edges, F32)[:len(pos)]
    return flat.reshape(M, C)


def resample_hand_filters(rs, integer):
    """the hand-built filters of CASES['resample_filters'] packed as the entry point takes them: (filters [nf, 6] int64,
    weights fp32); base such that the first taps fall before sample 0"""
    rows, chunks, woff = [], [], 0
    for taps, P, Q in CASES["resample_filters"]:
        w = rs.randint(-3, 4, (P, taps)).astype(F32) if integer else rfull(rs, (P, taps), -3, 1)
        rows.append([P, Q, taps, taps // 2, woff, 0])
        chunks.append(w.reshape(-1))
        woff += w.size
    return np.array(rows, np.int64), np.concatenate(chunks)


def n_in_for_valid(n_valid, P, Q):
    """the smallest n_in with floor(n_in P / Q) == n_valid"""
    return -(-n_valid * Q // P)


# ------------------------------------------------------------------ mel_nnls_pg
PG_MAX_BINS, PG_MAX_MELS = 1024, 128


def mel_tables(nbp, C, rs, integer):
    """A sparse mel basis in the form dvae_mel_nnls_pg takes: bin j < nb has the primary filter p(j) = j C // nb in slot 0
    and, in the second half of its group, the next filter in slot 1; filter f's bin range is then contiguous and every bin
    inside it names f.  The last 3 bins of nbp >= 8 lie under no filter (-1, weights NaN: never used).  -> (filt_range
    [C, 2] int32, bin_filt [nbp, 2] int32, bin_w [nbp, 2] fp32, dense [C, nbp] float64)"""
    nb = nbp - 3 if nbp >= 8 else nbp
    assert C <= nb
    p = np.arange(nb) * C // nb
    bf = np.full((nbp, 2), -1, np.int32)
    bw = np.full((nbp, 2), np.nan, F32)
    dense = np.zeros((C, nbp))
    for j in range(nb):
        grp = np.nonzero(p == p[j])[0]
        second = p[j] + 1 < C and j >= grp[0] + (len(grp) + 1) // 2
        w = rs.randint(1, 3, 2).astype(F32) if integer else (0.05 + 0.5 * rs.rand(2)).astype(F32)
        bf[j, 0], bw[j, 0] = p[j], w[0]
        dense[p[j], j] = w[0]
        if second:
            bf[j, 1], bw[j, 1] = p[j] + 1, w[1]
            dense[p[j] + 1, j] = w[1]
    fr = np.zeros((C, 2), np.int32)
    for f in range(C):
        js = np.nonzero(dense[f])[0]
        fr[f] = (js[0], js[-1] + 1)
        assert np.array_equal(js, np.arange(js[0], js[-1] + 1))
    return fr, bf, bw, dense


def nnls_step(x, amp, fr, bf, bw, step, dtype=F64, fma=False):
    """one projected-gradient step of every row in the kernel's order -> (x', tol of this step given x; dtype float64 only)"""
    x, amp = np.asarray(x, dtype), np.asarray(amp, dtype)
    rows, nbp = x.shape
    C = len(fr)
    w = np.asarray(bw, dtype)
    step = dtype(F32(step))

    def mac(acc, a, b):
        if dtype is F64:
            return acc + a * b
        return (acc.astype(F64) + a.astype(F64) * b.astype(F64)).astype(F32) if fma else acc + a * b
    r, ra = -amp.copy(), np.abs(amp).astype(F64)
    for f in range(C):
        for j in range(fr[f, 0], fr[f, 1]):
            wj = w[j, 0] if bf[j, 0] == f else w[j, 1]
            r[:, f] = mac(r[:, f], np.full(rows, wj, dtype), x[:, j])
            ra[:, f] += np.abs(F64(wj) * x[:, j].astype(F64))
    k = (fr[:, 1] - fr[:, 0] + 1).astype(F64)
    dr = g(k)[None, :] * ra                                              # |r - float64 r| of a k-term chain from -a
    out, tol = x.copy(), np.full(x.shape, FLOOR)
    for j in range(nbp):
        f0, f1 = bf[j]
        if f0 < 0:
            continue
        gj = w[j, 0] * r[:, f0]
        dg = np.abs(F64(w[j, 0])) * dr[:, f0] + g(2) * np.abs(gj.astype(F64))
        if f1 >= 0:
            gj = mac(gj, np.full(rows, w[j, 1], dtype), r[:, f1])
            dg = dg + np.abs(F64(w[j, 1])) * dr[:, f1] + g(2) * np.abs(F64(w[j, 1]) * r[:, f1].astype(F64))
        pre = mac(x[:, j], np.full(rows, -step, dtype), gj)
        out[:, j] = np.maximum(dtype(0), pre)
        tol[:, j] = (F64(step) * dg + g(2) * np.abs(F64(step) * gj.astype(F64)) + EPS32 * np.abs(pre.astype(F64))) * (1 + g(4)) + FLOOR
    return out, tol


def nnls_bounds(x, amp, fr, bf, bw, step, iters):
    """(x after `iters` steps in float64, per-element tol of the LAST step alone (what iters = 1 is held to), bound of each
    row's 2-norm error).  The map x -> max(0, x - step M^T (M x - a)) is non-expansive in the 2-norm for step <= 1 / |M|^2
    (I - step M^T M has its spectrum in [0, 1], the projection onto x >= 0 is non-expansive), so an error made in one step
    is not amplified by the later ones: the row's error after k steps is at most the sum of the 2-norms of the per-step
    bounds, each taken along the float64 trajectory (the difference to the device's own trajectory is of second order and
    covered by the factor 1 + 2^-10)."""
    x = np.asarray(x, F64)
    norm2, tol = np.zeros(x.shape[0]), np.zeros(x.shape)
    for _ in range(iters):
        x, tol = nnls_step(x, amp, fr, bf, bw, step)
        norm2 += np.sqrt((tol ** 2).sum(1))
    return x, tol, norm2 * (1 + 2.0 ** -10)


def nnls_f32(x, amp, fr, bf, bw, step, iters, fma):
    x = f32(x)
    for _ in range(iters):
        x, _ = nnls_step(x, amp, fr, bf, bw, step, F32, fma)
    return x


# ------------------------------------------------------------------ volume_normalize
NV_THREADS, NV_PER, NV_TILE = 256, 8, 2048


def volume_table(n_outs):
    """(segs [nseg, 6] int64 (only out0, n_out matter), tiles [ntiles, 2], tile_first [nseg + 1])"""
    segs, tiles, first, out0 = [], [], [0], 0
    for s, n in enumerate(n_outs):
        segs.append([0, n, out0, n, n, 0])
        tiles += [[s, t0] for t0 in range(0, n, NV_TILE)]
        first.append(len(tiles))
        out0 += (n + 3) // 4 * 4
    return np.array(segs, np.int64), np.array(tiles, np.int64), np.array(first, np.int64)


def volume_bounds(y, segs, tiles, tile_first, target_dbfs, increase_only):
    """dict(part: the float64 partials in the DOCUMENTED order (thread: its 8 samples in order; then the fixed halving tree
    over 256 threads), which is bit-determined because the square of an fp32 value is exact in float64, fused or not;
    part_sum (math.fsum) and tol_part = 17 u part (7 + 8 additions, compounded); ms (in order), ms_true, tol_ms;
    gain float64, tol_gain; silent).
    gain = fl32(pow(10, (target - 10 log10 ms) / 20)) in float64 on the device.  With u = 2^-53 and float64 log10 / pow
    within 2 u relative: change = target - 10 log10 ms carries 4 u (|target| + |10 log10 ms| + |change|), the exponent
    change / 20 one more, so gain's relative error before the final rounding is at most
    rel = ln10 / 20 * 5 u (|target| + |10 log10 ms| + |change|) + 4 u, plus 1/2 of ms's own relative error (gain ~ ms^-1/2);
    the final rounding to fp32 adds eps32: tol_gain = gain (eps32 + rel + tol_ms / (2 ms)) (1 + 2^-20)."""
    import math
    u = 2.0 ** -53
    y = np.asarray(y, F32)
    part, part_sum = [], []
    for s, t0 in np.asarray(tiles, np.int64):
        out0, n_out = int(segs[s][2]), int(segs[s][3])
        v = np.zeros(NV_TILE)
        m = min(NV_TILE, n_out - t0)
        v[:m] = y[out0 + t0:out0 + t0 + m].astype(F64)
        sq = (v * v).reshape(NV_THREADS, NV_PER)
        acc = np.zeros(NV_THREADS)
        for e in range(NV_PER):
            acc = acc + sq[:, e]
        h = NV_THREADS // 2
        while h:
            acc[:h] = acc[:h] + acc[h:2 * h]
            h //= 2
        part.append(acc[0])
        part_sum.append(math.fsum((v * v).tolist()))
    part, part_sum = np.array(part), np.array(part_sum)
    nseg = len(segs)
    ms, ms_true, tol_ms = np.zeros(nseg), np.zeros(nseg), np.zeros(nseg)
    for s in range(nseg):
        a, b, n = int(tile_first[s]), int(tile_first[s + 1]), int(segs[s][3])
        acc = 0.0
        for i in range(a, b):
            acc = acc + part[i]
        ms[s] = acc / n if n > 0 else 0.0
        ms_true[s] = math.fsum(part_sum[a:b].tolist()) / n if n > 0 else 0.0
        tol_ms[s] = (17 + (b - a) + 1) * u * ms_true[s] * (1 + 2.0 ** -20)
    gain, tol_gain, silent = np.ones(nseg), np.zeros(nseg), np.zeros(nseg, np.int32)
    for s in range(nseg):
        if not ms_true[s] > 0:
            silent[s] = 1
            continue
        l10 = 10.0 * math.log10(ms_true[s])
        change = target_dbfs - l10
        if increase_only and change < 0:
            continue
        gain[s] = 10.0 ** (change / 20.0)
        rel = math.log(10.0) / 20.0 * 5 * u * (abs(target_dbfs) + abs(l10) + abs(change)) + 4 * u
        tol_gain[s] = gain[s] * (EPS32 + rel + tol_ms[s] / (2 * ms_true[s])) * (1 + 2.0 ** -20)
    return dict(part=part, part_sum=part_sum, tol_part=17 * u * part_sum * (1 + 2.0 ** -20), ms=ms, ms_true=ms_true,
                tol_ms=tol_ms, gain=gain, tol_gain=tol_gain, silent=silent)


# ------------------------------------------------------------------ f0_viterbi
F0_STATES, F0_BACK_LD, F0_CHUNK = 206, 208, 256


def viterbi_ref(r, gain, voiced, segs, l2, oct_, jump, rate, lag_min, last_on_tie=False):
    """dvae_f0_viterbi in float64, every operation rounded once in the order the header gives: per maximal run of voiced
    frames s = r gain / r(0) - oct, D = s at the first frame, D_k(j) = s_k(j) + max_i (D_{k-1}(i) - jump |l2[j] - l2[i]|), the
    first maximal i; the first arg-max of the last D starts the traceback.  -> dict(lag int32 [rows], f0, tol_f0, lf0v (NaN
    where nothing is written), tol_lf0v, runs [(first row, last row)]).  f0 is rounded once from float64 (tol eps32 f0);
    lf0v = fl32(ln f0) of that fp32 value: one more rounding and float64 log's own error (4 u), and f0's rounding moves ln f0
    by eps32: tol = eps32 (1 + |ln f0|) + 8 u |ln f0|.  last_on_tie: the seeded mistake (>= for >)."""
    r64, gn = np.asarray(r, F64), np.asarray(gain, F64)
    rows = r64.shape[0]
    S = F0_STATES
    T = jump * np.abs(l2[:, None] - l2[None, :])                         # [j, i]
    lag, f0 = np.zeros(rows, np.int32), np.zeros(rows)
    lf = np.full(rows, np.nan)
    runs = []

    def amax(c):
        return c.shape[-1] - 1 - np.argmax(c[..., ::-1], axis=-1) if last_on_tie else np.argmax(c, axis=-1)
    for row0, M, _, _ in np.asarray(segs, np.int64):
        v = np.concatenate([[0], np.asarray(voiced[row0:row0 + M]) != 0, [0]]).astype(np.int8)
        d = np.diff(v)
        rank = 0
        for a, b in zip(np.nonzero(d == 1)[0], np.nonzero(d == -1)[0] - 1):
            runs.append((int(row0 + a), int(row0 + b)))
            rr = r64[row0 + a:row0 + b + 1]
            s = rr[:, 1:S + 1] * gn[None, 1:S + 1] / rr[:, :1] - oct_[None, :]
            K = b - a + 1
            D, back = s[0].copy(), np.zeros((K, S), np.int64)
            for k in range(1, K):
                cand = D[None, :] - T
                back[k] = amax(cand)
                D = s[k] + cand[np.arange(S), back[k]]
            st = np.zeros(K, np.int64)
            st[-1] = int(np.argmax(D))
            for k in range(K - 1, 0, -1):
                st[k - 1] = back[k, st[k]]
            for k in range(K):
                j, delta = int(st[k]), 0.0
                if 0 < j < S - 1:
                    q = rr[k, j:j + 3] * gn[j:j + 3]
                    den = q[0] - 2.0 * q[1] + q[2]
                    if den < 0:
                        delta = min(0.5, max(-0.5, 0.5 * (q[0] - q[2]) / den))
                row = row0 + a + k
                lag[row], f0[row] = lag_min + j, rate / ((lag_min + j) + delta)
                lf[row0 + rank + k] = np.log(F64(F32(f0[row])))
            rank += K
    u = 2.0 ** -53
    return dict(lag=lag, f0=f0, tol_f0=EPS32 * f0 + FLOOR, lf0v=lf, tol_lf0v=EPS32 * (1 + np.abs(lf)) + 8 * u * np.abs(lf) + FLOOR,
                runs=runs)


def viterbi_tables():
    """hand-built l2, oct (float64, [206]): l2 = j / 8 with the states of each tie pair sharing one value, oct small integers,
    0 at the designated winners and 32 at their neighbours (so a winner wins against a larger q next to it)"""
    j = np.arange(F0_STATES)
    l2 = j / 8.0
    oct_ = (j % 3).astype(F64)
    for a in VIT_PAIRS:
        l2[a + 1], oct_[a], oct_[a + 1] = l2[a], 0.0, 0.0
    for m in VIT_WINNERS.values():
        oct_[m] = 0.0
        for nb in (m - 1, m + 1):
            if 0 <= nb < F0_STATES:
                oct_[nb] = 32.0
    return l2, oct_


VIT_PAIRS = (17, 40)                                  # states a, a + 1 with identical scores on every frame
VIT_RUNS = (1, 2, 256, 257, 513)                      # one, one, one, two and three traceback chunks
# run -> winner state and (q(m-1), q(m), q(m+1)): the parabola at state 0 and 205 (no refinement), a non-concave triple
# (delta = 0), vertices beyond -1/2 and +1/2 (clamped), a vertex inside (0.1)
VIT_WINNERS = {"first_state": 0, "last_state": 205, "not_concave": 50, "clamp_low": 100, "clamp_high": 120, "inside": 150}
VIT_TRIPLES = {"first_state": (None, 8, 2), "last_state": (2, 8, None), "not_concave": (16, 8, 16), "clamp_low": (12, 8, 0),
               "clamp_high": (0, 8, 12), "inside": (2, 8, 4)}


def viterbi_e_case(ldr=209):
    """Class E: r small integers, gain in {1, 2}, r(0) in {1, 2}: s, D, the jump costs (jump a power of two, l2 multiples of
    1/8) are exact in float64, so lag is determined on every frame.  Three utterances: (0) runs of VIT_RUNS frames one
    unvoiced frame apart, the last ending on the last frame; the boosted states alternate between the tie pairs, so the path
    jumps and every decision on it is a tie that must go to the first state; (1) one 3-frame run per VIT_WINNERS entry;
    (2) no voiced frame.  -> r, gain, voiced, segs, expected deltas {row: delta} of utterance 1"""
    rs = np.random.RandomState(206)
    S = F0_STATES
    gain = np.full(ldr, np.nan, F32)
    gain[1:S + 1] = 2.0 ** rs.randint(0, 2, S)
    for a in VIT_PAIRS:
        gain[1 + a + 1] = gain[1 + a]
    v0 = []
    for n_ in VIT_RUNS:
        v0 += [1] * n_ + [0]
    v0 = v0[:-1]
    v1 = []
    for _ in VIT_WINNERS:
        v1 += [0, 1, 1, 1]
    v2 = [0] * 5
    Ms = [len(v0), len(v1), len(v2)]
    rows = sum(Ms)
    r = np.full((rows, ldr), np.nan, F32)
    r[:, 1:S + 1] = rs.randint(0, 3, (rows, S))
    r[:, 0] = 2.0 ** rs.randint(0, 2, rows)
    for k in range(Ms[0]):
        a = VIT_PAIRS[0] if k % 7 < 4 else VIT_PAIRS[1]
        r[k, 1 + a] += 8 + k % 2
        r[k, 1 + a + 1] = r[k, 1 + a]
    for a in VIT_PAIRS:
        r[:Ms[0], 1 + a + 1] = r[:Ms[0], 1 + a]
    for i, name in enumerate(VIT_WINNERS):
        m = VIT_WINNERS[name]
        for k in range(Ms[0] + 4 * i + 1, Ms[0] + 4 * i + 4):
            r[k, 0] = 1.0
            for off, q in zip((-1, 0, 1), VIT_TRIPLES[name]):
                if q is not None:
                    r[k, 1 + m + off] = q / gain[1 + m + off]
    return r, gain, np.array(v0 + v1 + v2, np.int32), seg_table(Ms, [0, 0, 0])


# ------------------------------------------------------------------ launch geometry of the simple kernels
def transpose_geometry(M, C):
    """the 32 x 32 LDS tiles of mel_db_normalize / mel_denormalize over [M or L, C]"""
    return dict(tiles=(-(-M // 32), -(-C // 32)), partial=(M % 32 != 0, C % 32 != 0))


def flat_geometry(work, per_block=256):
    """one thread per element (or per 4): blocks, and whether the last block is partly idle"""
    return dict(blocks=-(-work // per_block), idle_tail=work % per_block != 0)
