"""The exact reference of the contraction family (csrc/gemm.hip, csrc/gemm_common.h, csrc/gemm256.hip: every kernel behind
dvae_gemm_f32 / _batched / _slabs / _batched_slabs and the dvae_conv5_* entry points), the input classes it is held to, the
bounds of the one class that rounds, the cases, and a Python restatement of the dispatch.  Not a test module and no GPU code:
tests/test_gemm_ref.py proves the reference, the classes, the bounds and the restated dispatch on the CPU and runs the
mutants; tests/test_hip_gemm.py runs `CASES` on the device and asserts which kernel each of them reached.  A change here moves
what the GPU tests accept: the formulas are the ABI's (include/dvae_hip.h), the bounds are derived below, neither follows
what some kernel computes.

Every case is one or several LOGICAL products  out = epi(base, act(a [M, K] b [K, N] + bias [N]))  (`products`): a plain
GEMM is one, a batched launch one per product, a conv forward / data gradient one over the five taps laid side by side
along k (K' = 5 K, rows of a shifted by +-(tap - 2) N_seg frames-major rows, zero outside the sequence), a conv weight
gradient one per tap with the k rows of b shifted.  The operand layouts, leading dimensions, slabs and k-splits are how the
device is ASKED for that product and never enter the expected value.

Input classes (generators `e1`, `e2`, `e3`, `rclass`; exactness proved in tests/test_gemm_ref.py for every prefix sum in
forward, reverse and tile-blocked order):

E1  selection, bit-exact.  One operand is arbitrary fp32 (24 significand bits, exponents 2^-20 .. 2^20, so every split
    term stays normal); the other has ONE nonzero +-2^e, e in [-3, 3], per dot product, at k(j) = (s j + r) mod K for the
    offsets `e1_offsets`: every k of the product while K <= 6 min(M, N), else the first and last k-tile and both sides of
    the first four split boundaries (a conv forward / data gradient walks its 5 C taps with s = C + 1).  The result is +-2^e x bit for bit:
    fp32x3 needs all of x1 b1, x2 b1, x3 b1; the bf16 mode returns 2^e rne_bf16(x).  A lost, doubled or mis-addressed term
    returns another operand's bits.
E2  small integers, bit-exact and dense: |a|, |b| <= 15, integer bias and base, K 225 + |bias| + |base| < 2^24: every
    partial sum in every order is an integer below 2^24, so every arithmetic, atomics, slabs and their folds, batched
    launches and the ReLU epilogue equal the integer product exactly.
E3  two-term integers, bit-exact in fp32 and fp32x3: odd |a|, |b| < 2^10 (two bf16 terms each), one operand dense, the other
    with at most 8 nonzeros per dot product: |sum| < 2^23.  Needs a1 b2, a2 b1 and a2 b2 as well.
R   the rounding class: full-significand values, one row block of a scaled by 2^-12 and one column block of b by 2^+12 (a
    max norm would hide either), bias and base as wide, a zero row block of a whose outputs must equal epi(base, act(bias))
    exactly.

Bounds of class R (eps = 2^-24).  S_ij = sum_k |a_ik b_kj| + |bias_j| + |base_ij|.  A worst-case g(K) S is useless at
K = 512 .. 8192, so the constants are MEASURED on the reference side: `restate` evaluates the arithmetic from its definition
(include/dvae_hip.h, gemm_common.h) in numpy fp32 —
    fp32    rounded products, accumulated in fp32;
    fp32x3  the three-term split and the six partial products (each exact in fp32), accumulated in fp32;
    bf16    the float64 product of the RNE-rounded operands is the reference itself, so only the fp32 accumulation is left to
            bound; its constants are those of the fp32 restatement of the same, UNROUNDED operands (see below)
— in two orders, left to right and in k-tiles of 16 (a tile's partial sum formed first, then added), on `sample_rows_cols`
(the first and last row / column of every tile edge and every row / column of the scaled blocks; every element of a small
case).  rho_max, rho_rms = the
worst and the RMS |err| / S of the two orders against float64.  The device must keep
        |err_ij| <= 2 rho_max S_ij  at EVERY element      and      RMS(err / S) <= 2 rho_rms  over the whole output
(rho_max of a SAMPLE is first carried to the size of the output: the worst of n draws of a near-normal error grows as
sqrt(2 ln n), so rho_max is multiplied by sqrt(ln(M N) / ln(sample size)) — 1 for a fully restated case, 1.44 at most; with
the sample's own worst the fp32 kernels, whose fmaf chain has the statistics of the restatement itself (RMS at 0.5 of its
limit), exceeded 2 rho_max S by 1.06 - 1.19 at 8 elements of three outputs of 0.5 to 34 million: xcd-8x7, xcd-24x7,
big-kr-ragged)
— the factor 2 on each side is the margin tests/lstm_ref.py uses for its recurrent product: the kernel's order (the order
inside an MFMA, taps inside k-tiles) is neither of the two restated; rho_max >= eps / 2 and rho_rms >= eps / 4, one rounding
of the last sum, where both restated orders happen to be exact.  fp32x3 is measured against its OWN restatement (six
terms per k make rho about 3 x that of plain fp32; a plain-fp32 rho would fail a correct kernel).  Epilogues: the bias and
the base are part of the restatement (one rounding each); an atomic k-split or EPI_ACCUM rounds (base + partial) once per
writer in an order of the hardware's choosing: + eps (|base| + S) per split, the form DESIGN.md section 5 gives for dbias.
tanh: sech^2(max(|u| - tol_u, 0)) tol_u + TANHF_ROUNDINGS eps |tanh u| with tests/bn_ref.py's measured TANHF_ROUNDINGS; a
bf16 store (c16): + 2^-8 (|z| + tol).  The RMS condition: over the whole output without an activation, over the elements
with u > 2 rho_max S (which ReLU passes unchanged whatever the error) with ReLU; tanh and the bf16 store are held per
element only — their own rounding (TANHF_ROUNDINGS eps, 2^-8) is far above rho_rms and would be all the RMS measures.
Under tanh the exact classes are exact BEFORE the activation only: the result is held to TANHF_ROUNDINGS eps |tanh u| there.
The accumulation constant of the bf16 mode, corrected by its derivation.  Restating "exact products of the rounded operands,
accumulated in fp32" measures nothing: two 8-bit significands give a 16-bit product, and nearly every fp32 add of such terms
is EXACT (rho_max = rho_rms = 0 up to K of several hundred), a constant no accumulator is bound to that aligns its addends to
the running sum and drops what falls below its last place — which is what the matrix cores do: on the 256 x 128 bf16 tile at
K = 512 the device is exact to the last rounding at 94 % of 6.3 million elements (RMS |err| / S = 0.036 eps) and off by up to
8.5 units in the last place of the result where |result| is largest (1.72 eps S at the worst of them).  Each add may lose up
to one unit in the last place of the running sum whether or not the addend had bits to spare, which is the behaviour of an
accumulation in which EVERY add rounds: the fp32 restatement of the same operands before their rounding to bf16 (24-bit
significands, a rounded product and a rounded sum per term).  Its rho_max, rho_rms are the bf16 mode's constants; the
reference stays the float64 product of the rounded operands, and the factor 2 stays.  (Borrowed from another arithmetic, this
constant is not tight — the device stays below 0.4 of it on the tall bf16 tile; a restatement that models the matrix cores'
truncating alignment of the addends would give the bf16 mode a constant of its own.)

What the RMS condition can see: a lost a1 b3 term moves rho_rms to 12.7 / 5.7 / 2.3 x 2^-24 at K = 16 / 80 / 516 against 0.9
of the intact restatement (tests/test_gemm_ref.py) — its share falls as 1 / sqrt(K).  On the restatement class R flags it
at K = 16 at every element, at K = 516 through the RMS alone and barely (2.1 against 1.7 eps), not at K = 2048; the device
accumulates more accurately than the restatement, so there the RMS condition should be trusted up to K of about 80 only.
Beyond that a lost split term is found by E1 and E3, which flag it at every K.
"""
import collections
import zlib

import numpy as np

from ref_common import (ACT_NONE, ACT_RELU, ACT_TANH, BF16_REL, EPS32, F, F64, MODE_BF16, MODE_F32, MODE_F32X3, bf16,  # noqa: F401
                        bf16_trunc, split3)

A_BF16, B_BF16, C_BF16 = 0x100, 0x200, 0x400
EPI_STORE, EPI_ACCUM, EPI_ATOMIC = 0, 1, 2
MODES = {"fp32": MODE_F32, "bf16": MODE_BF16, "fp32x3": MODE_F32X3}
TAPS = 5


# ----------------------------------------------------------------------------------------------------------- arithmetic
X3_TERMS = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))      # a1b1 a1b2 a2b1 a2b2 a1b3 a3b1: weight >= 2^-16


def operand(v, mode):
    """An operand as the mode's products take it (fp32 values)."""
    return bf16(v) if mode == MODE_BF16 else np.asarray(v, F)


def act_apply(u, act):
    return np.maximum(u, 0) if act == ACT_RELU else np.tanh(u) if act == ACT_TANH else u


def terms_of(a, b, mode, drop=None, trunc=False):
    """The (a-plane, b-plane) pairs whose exact fp32 products one k step accumulates."""
    if mode == MODE_F32:
        return [(np.asarray(a, F), np.asarray(b, F))]
    if mode == MODE_BF16:
        r = bf16_trunc if trunc else bf16
        return [(r(a), r(b))]
    pa, pb = split3(a), split3(b)
    return [(pa[i], pb[j]) for i, j in X3_TERMS if (i, j) != drop]


def restate(a, b, mode, order, bias=None, base=None, k_per_split=None, mut=None):
    """epi(base, a b + bias) in the arithmetic of `mode`, every operation rounded to fp32, k cut into splits of k_per_split
    (the bias rides split 0, the splits are added to the base in order).  order "seq": left to right; "tile": k-tiles of 16,
    a tile's partial sum first.  `mut`: a mutation of tests/test_gemm_ref.py (dict)."""
    mut = mut or {}
    a, b = np.asarray(a, F), np.asarray(b, F)
    M, K = a.shape
    N = b.shape[1]
    terms = terms_of(a, b, mode, drop=mut.get("drop"), trunc=mut.get("trunc", False))
    kps = k_per_split or K
    out = None if base is None or mut.get("no_base") else np.asarray(base, F).copy()
    for s, k0 in enumerate(range(0, K, kps)):
        k1 = min(K, k0 + kps)
        if mut.get("double_tile") and s > 0:
            k0 -= 16                                   # the split re-reads its neighbour's last k-tile
        acc = np.zeros((M, N), F)
        ks = [k for k in range(k0, k1) if k != mut.get("skip_k")]
        if order == "seq":
            for k in ks:
                for ta, tb in terms:
                    acc += ta[:, k:k + 1] * tb[k]
        else:
            for t0 in range(0, len(ks), 16):
                for ta, tb in terms:
                    part = np.zeros((M, N), F)
                    for k in ks[t0:t0 + 16]:
                        part += ta[:, k:k + 1] * tb[k]
                    acc += part
                if mut.get("acc_bf16"):
                    acc = bf16(acc)
        if bias is not None and (s == 0 or mut.get("bias_per_split")):
            acc = acc + np.asarray(bias, F)
        out = acc if out is None else (out + acc).astype(F)
    return out


def shift_rows(x, d):
    """y[r] = x[r + d], zero outside the matrix (the conv padding on frame-major rows)."""
    y = np.zeros_like(x)
    R = x.shape[0]
    if d >= 0:
        y[:max(R - d, 0)] = x[d:]
    else:
        y[-d:] = x[:max(R + d, 0)]
    return y


def cat_taps(x, nshift):
    """[R, C] -> [R, 5 C]: tap-major along k, tap's block = the rows shifted by (tap - 2) nshift."""
    return np.concatenate([shift_rows(x, (t - 2) * nshift) for t in range(TAPS)], axis=1)


# ----------------------------------------------------------------------------------------------------------- the cases
_FIELDS = dict(name="", entry="gemm", M=0, N=0, K=0, a_kc=True, b_kc=True, mode="fp32x3", a16=False, b16=False, c16=False,
               bias=False, act=ACT_NONE, epi=EPI_STORE, split=1, slab_cap=None, batch=1, shared_b=False, ldc_pad=0, c_off=0,
               nseg=0, G=0, deterministic=False, classes=("E1", "E2", "E3", "R"), use_fold=False, reach=None)
Case = collections.namedtuple("Case", list(_FIELDS), defaults=list(_FIELDS.values()))
CONV_ENTRIES = ("conv_fwd", "conv_fwd_stats", "conv_dgrad", "conv_wgrad", "conv_fwd_slabs", "conv_dgrad_slabs",
                "conv_wgrad_slabs")


def is_conv(c):
    return c.entry in CONV_ENTRIES


def is_wgrad(c):
    return c.entry in ("conv_wgrad", "conv_wgrad_slabs")


def logical_dims(c):
    """(M, N, K) of the logical product(s): a [M, K], b [K, N].  A conv forward / data gradient concatenates its taps."""
    if is_conv(c) and not is_wgrad(c):
        return c.M, c.N, TAPS * c.K
    return c.M, c.N, c.K


def n_outputs(c):
    return TAPS if is_wgrad(c) else c.batch


def tap_shift(c):
    """rows of the activation operand per (tap - 2): +N_seg forward and weight gradient, -N_seg data gradient."""
    return -c.nseg if c.entry in ("conv_dgrad", "conv_dgrad_slabs") else c.nseg


def products(c, a, b):
    """The logical (a_eff, b_eff) of every output of the case from its generated operands.
    gemm: a [M, K], b [K, N];  batched: lists of them;  conv forward / data gradient: a = the activation rows [R, C], b =
    the taps side by side [5 C, Nout];  weight gradient: a = dY^T [Cout, R], b = X [R, Cin]."""
    if is_wgrad(c):
        return [(a, shift_rows(b, (t - 2) * tap_shift(c))) for t in range(TAPS)]
    if is_conv(c):
        return [(cat_taps(a, tap_shift(c)), b)]
    if c.batch > 1:
        return list(zip(a, b))
    return [(a, b)]


def has_base(c):
    return c.epi != EPI_STORE


def mm_exact(a, b):
    """The product of operands whose every partial sum is an integer multiple of one power of two below 2^24 units: float64
    holds it exactly whatever the order (asserted in tests/test_gemm_ref.py against int64)."""
    return np.asarray(a, F64) @ np.asarray(b, F64)


def mm_exact_f32(a, b):
    """The same through the fp32 BLAS product — exact for E2 / E3 too, the reference of the large cases."""
    import torch
    return (torch.from_numpy(np.ascontiguousarray(a, F)) @ torch.from_numpy(np.ascontiguousarray(b, F))).numpy()


def want_u(c, a, b, bias, big=False):
    """the exact pre-activation of E1 / E2 / E3 in float64"""
    mode = MODES[c.mode]
    u = (mm_exact_f32 if big else mm_exact)(operand(a, mode), operand(b, mode)).astype(F64)
    return u if bias is None else u + bias


def expected_exact(c, a, b, bias, base, big=False):
    """E1 / E2 / E3: the value every arithmetic must return bit for bit (operands rounded first in the bf16 mode)."""
    mode = MODES[c.mode]
    mm = mm_exact_f32 if big else mm_exact
    u = mm(operand(a, mode), operand(b, mode))
    if bias is not None:
        u = u + bias
    z = act_apply(u, c.act)
    if base is not None:
        z = z + base
    z = np.asarray(z, F)
    return bf16(z) if c.c16 else z


# ----------------------------------------------------------------------------------------------------------- input classes
def rng_of(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def full_sig(rs, shape, emin, emax):
    """fp32 values with all 24 significand bits in use (the lowest one set), exponents uniform in [emin, emax], random sign."""
    m = (rs.integers(0, 1 << 23, shape, dtype=np.int64) | 1) + (1 << 23)
    e = rs.integers(emin, emax + 1, shape)
    sg = rs.integers(0, 2, shape) * 2 - 1
    return (sg * m.astype(F64) * np.exp2(e - 23.0)).astype(F)


def e1_offsets(K, n, k_per_split, bk):
    """Offsets r of k(j) = (j + r) mod K, j < n.  While ceil(K / n) <= 6 the windows [r, r + n) tile the whole of k: EVERY k
    is selected once — every k-tile and both sides of every split boundary.  A longer k (a few cases with K >= 8 n) keeps
    the first k-tile, the last (partial) k-tile and both sides of the first four split boundaries; the dense classes cover
    the addressing of the rest."""
    if -(-K // n) <= 6:
        rs = list(range(0, K, n))
    else:
        rs = [0, (K - n) % K] + [(kb - min(n, 2 * bk) // 2) % K for kb in list(range(k_per_split, K, k_per_split))[:4]]
    out = []
    for r in rs:
        if r not in out:
            out.append(r)
    return out


def e1(key, M, N, K, role, r, s=1):
    """role "B": a arbitrary, column j of b has its nonzero at k = (s j + r) mod K; role "A": row i of a at k = (s i + r) mod K."""
    rs = rng_of("E1", key, role, r)
    if role == "B":
        a = full_sig(rs, (M, K), -20, 20)
        b = np.zeros((K, N), F)
        j = np.arange(N)
        b[(s * j + r) % K, j] = (rs.integers(0, 2, N) * 2 - 1) * np.exp2(rs.integers(-3, 4, N))
    else:
        b = full_sig(rs, (K, N), -20, 20)
        a = np.zeros((M, K), F)
        i = np.arange(M)
        a[i, (s * i + r) % K] = (rs.integers(0, 2, M) * 2 - 1) * np.exp2(rs.integers(-3, 4, M))
    return a, b


def e2(key, M, N, K, bias, base, amp=15):
    """amp = 1 (bias within +-3): the outputs stay so small that 64 of their SQUARES sum exactly in fp32 too (the BatchNorm
    statistics epilogue of dvae_conv5_fwd_stats; the test asserts 64 max y^2 < 2^24 on the outputs it got)."""
    rs = rng_of("E2", key)
    a = rs.integers(-amp, amp + 1, (M, K)).astype(F)
    b = rs.integers(-amp, amp + 1, (K, N)).astype(F)
    nb = 1000 if amp > 1 else 3
    bi = rs.integers(-nb, nb + 1, N).astype(F) if bias else None
    ba = rs.integers(-100000, 100001, (M, N)).astype(F) if base else None
    assert K * amp * amp + nb + 100000 < 1 << 24
    return a, b, bi, ba


def e3(key, M, N, K, role, r, s=1):
    """role = the SPARSE operand (<= 8 nonzeros per dot product, at (s i + r + t step) mod K); the other one is dense."""
    rs = rng_of("E3", key, role, r)
    odd = lambda shape: ((2 * rs.integers(0, 512, shape) + 1) * (rs.integers(0, 2, shape) * 2 - 1)).astype(F)
    nz = min(8, K)
    step = max(1, K // 8)
    if role == "B":
        a, full = odd((M, K)), odd((K, N))
        b = np.zeros((K, N), F)
        j = np.arange(N)
        for t in range(nz):
            k = (s * j + r + t * step) % K
            b[k, j] = full[k, j]
    else:
        b, full = odd((K, N)), odd((M, K))
        a = np.zeros((M, K), F)
        i = np.arange(M)
        for t in range(nz):
            k = (s * i + r + t * step) % K
            a[i, k] = full[i, k]
    return a, b


def r_blocks(M, N):
    """(zero rows, rows scaled 2^-12, columns scaled 2^+12) as slices: 16-wide blocks where the matrix is large enough."""
    zr = slice(48, 64) if M >= 64 else slice(M - max(1, M // 4), M)
    sr = slice(16, 32) if M >= 64 else slice(0, max(1, M // 4))
    sc = slice(8, 24) if N >= 24 else slice(0, max(1, N // 4))
    return zr, sr, sc


def rclass(key, M, N, K, bias, base):
    rs = rng_of("R", key)
    a, b = full_sig(rs, (M, K), -1, 1), full_sig(rs, (K, N), -1, 1)
    zr, sr, sc = r_blocks(M, N)
    a[sr] *= F(2.0 ** -12)
    b[:, sc] *= F(2.0 ** 12)
    a[zr] = 0
    rowsc, colsc = np.ones((M, 1), F), np.ones(N, F)
    rowsc[sr] = 2.0 ** -12
    colsc[sc] = 2.0 ** 12
    bi = full_sig(rs, (N,), -1, 3) * colsc if bias else None
    ba = full_sig(rs, (M, N), -1, 3) * rowsc * colsc if base else None
    return a, b, bi, ba


# ----------------------------------------------------------------------------------------------------------- bounds of R
def sample_idx(n, tile, every):
    """first and last index of every tile edge (all of them when `every`)"""
    if every:
        return np.arange(n)
    s = {0, n - 1}
    for t in range(tile, n, tile):
        s.update((t - 1, t))
    return np.array(sorted(s))


def sample_rows_cols(M, N, bm, bn):
    """The rows and columns the restatement runs on: every one of a small case; else the first and last of every tile edge
    (thinned to about 64 keeping the ends) and EVERY row and column of the scaled blocks of class R (`r_blocks`) — where the
    products are 2^-12 of the bias and the base, the roundings of the epilogue and of a slab sum are the whole error, and a
    sample without those rows would measure a constant that does not cover them."""
    if M * N <= 16384:
        return np.arange(M), np.arange(N)
    rows, cols = sample_idx(M, bm, False), sample_idx(N, bn, False)
    rows = rows[np.unique(np.linspace(0, len(rows) - 1, min(len(rows), 64)).astype(int))]
    cols = cols[np.unique(np.linspace(0, len(cols) - 1, min(len(cols), 64)).astype(int))]
    zr, sr, sc = r_blocks(M, N)
    rows = np.unique(np.concatenate([rows, np.arange(M)[sr], np.arange(M)[zr][[0, -1]]]))
    cols = np.unique(np.concatenate([cols, np.arange(N)[sc]]))
    return rows, cols


TANHF_ROUNDINGS = None      # tests/bn_ref.py's (imported lazily: both modules live in tests/)


def _tanhf_roundings():
    global TANHF_ROUNDINGS
    if TANHF_ROUNDINGS is None:
        import bn_ref
        TANHF_ROUNDINGS = bn_ref.TANHF_ROUNDINGS
    return TANHF_ROUNDINGS


def r_reference(c, a, b, bias, base):
    """float64 reference u = a b + bias (operands as the mode takes them), z = epi(base, act(u)), S."""
    mode = MODES[c.mode]
    a64, b64 = operand(a, mode).astype(F64), operand(b, mode).astype(F64)
    u = a64 @ b64
    S = np.abs(a64) @ np.abs(b64)
    if bias is not None:
        u = u + bias.astype(F64)
        S = S + np.abs(bias.astype(F64))
    z = act_apply(u, c.act)
    if base is not None:
        z = z + base.astype(F64)
        S = S + np.abs(base.astype(F64))
    return u, z, S


def rho_of(c, a, b, bias, base, k_per_split, bm, bn, mut=None, orders=("seq", "tile")):
    """rho_max, rho_rms of the restated arithmetic (pre-activation, with base) on the sample; worst of the orders."""
    M, N = a.shape[0], b.shape[1]
    rows, cols = sample_rows_cols(M, N, bm, bn)
    # bf16 mode: the accumulation is measured on the UNROUNDED operands in the fp32 arithmetic (see the module docstring)
    mode = MODE_F32 if MODES[c.mode] == MODE_BF16 else MODES[c.mode]
    sa, sb = a[rows], b[:, cols]
    sbias = None if bias is None else bias[cols]
    sbase = None if base is None else base[np.ix_(rows, cols)]
    a64, b64 = operand(sa, mode).astype(F64), operand(sb, mode).astype(F64)
    ref = a64 @ b64 + (0 if sbias is None else sbias.astype(F64)) + (0 if sbase is None else sbase.astype(F64))
    S = np.abs(a64) @ np.abs(b64) + (0 if sbias is None else np.abs(sbias.astype(F64))) + \
        (0 if sbase is None else np.abs(sbase.astype(F64)))
    live = S > 0
    rmax = rrms = 0.0
    for order in orders:
        got = restate(sa, sb, mode, order, sbias, sbase, k_per_split, mut).astype(F64)
        q = np.abs(got - ref)[live] / S[live]
        rmax, rrms = max(rmax, float(q.max())), max(rrms, float(np.sqrt(np.mean(q * q))))
    # Floor: where both restated orders happen to be EXACT (bf16-mode products of a few significant bits at small K) the
    # measured constants are 0, which no other order is bound to: an fp32 accumulation may always round its last sum once,
    # eps |result| <= eps S.  2 rho_max S and 2 rho_rms are never below that one rounding (RMS of one rounding: eps / 2).
    # Sample against population.  The worst of n_s restated elements is not the yardstick of the worst of n_d >= n_s device
    # elements: an error that is the sum of K independent roundings is close to normal, and the expected maximum of n draws
    # of one grows as sqrt(2 ln n).  rho_max is carried from the sample to the whole output by that factor (1 where every
    # element is restated; 1.44 from 64 x 64 samples to the 8192 x 4096 outputs); rho_rms needs none.
    n_s, n_d = len(rows) * len(cols), M * N
    grow = float(np.sqrt(np.log(max(n_d, n_s)) / np.log(max(n_s, 2))))
    return max(rmax * grow, EPS32 / 2), max(rrms, EPS32 / 4)


def r_bounds(c, a, b, bias, base, n_split, rho_max):
    """(z, tol, S, u): the float64 result, the per-element bound, the magnitude sum and the pre-activation."""
    u, z, S = r_reference(c, a, b, bias, base)
    tol = 2.0 * rho_max * S
    if c.epi != EPI_STORE:
        tol = tol + max(1, n_split) * EPS32 * S
    if c.act == ACT_TANH:
        tol = tol / np.cosh(np.minimum(np.maximum(np.abs(u) - tol, 0.0), 300.0)) ** 2 + _tanhf_roundings() * EPS32 * np.abs(np.tanh(u))
    if c.c16:
        tol = tol + BF16_REL * (np.abs(z) + tol)
    return z, tol, S, u


def r_check(c, got, a, b, bias, base, n_split, rho_max, rho_rms):
    """Failures (strings) of a device result `got` [M, N] of class R, and (worst err / tol, rms / (2 rho_rms))."""
    z, tol, S, u = r_bounds(c, a, b, bias, base, n_split, rho_max)
    got = np.asarray(got, F64)
    err = np.abs(got - z)
    fails = []
    zr = ~np.asarray(a, F).any(axis=1)          # rows of a that are all zero
    zexp = np.zeros(got.shape[1], F) if bias is None else np.asarray(bias, F)
    zexp = np.broadcast_to(np.asarray(act_apply(zexp.astype(F64), c.act), F) if c.act != ACT_TANH else zexp, got[zr].shape)
    if c.act != ACT_TANH and not c.c16 and zr.any():
        want = zexp if base is None else (np.asarray(base, F)[zr] + zexp).astype(F)
        if not np.array_equal(np.asarray(got[zr], F), want):
            fails.append(f"zero rows of a: {int((np.asarray(got[zr], F) != want).sum())} elements differ from epi(base, act(bias))")
    live = S > 0
    if np.any(got[~live] != 0):
        fails.append("an element with S = 0 is not exactly 0")
    ratio = np.zeros_like(err)
    ratio[live] = err[live] / np.maximum(tol[live], 1e-300)
    worst = float(ratio.max()) if live.any() else 0.0
    if worst > 1.0:
        i, j = np.unravel_index(np.argmax(ratio), ratio.shape)
        fails.append(f"element ({i}, {j}): |err| {err[i, j]:.3e} > bound {tol[i, j]:.3e} ({worst:.2f} x), {int((ratio > 1).sum())} over")
    rms_rel = 0.0
    if c.act == ACT_RELU:       # the RMS over the elements ReLU passes whatever the error: u beyond its own tolerance
        live = live & (u > 2.0 * rho_max * S)
    if c.act != ACT_TANH and not c.c16 and live.any():
        rms = float(np.sqrt(np.mean((err[live] / S[live]) ** 2)))
        lim = 2.0 * rho_rms + (max(1, n_split) * EPS32 if c.epi != EPI_STORE else 0.0)
        rms_rel = rms / lim
        if rms > lim:
            fails.append(f"RMS |err| / S = {rms / EPS32:.3f} eps > 2 rho_rms = {lim / EPS32:.3f} eps")
    return fails, worst, rms_rel


def exact_check(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and np.array_equal(got.view(np.uint32) if got.dtype == F else got,
                                                  want.view(np.uint32) if want.dtype == F else want):
        return []
    if got.shape != want.shape:
        return [f"{what}: shape {got.shape} != {want.shape}"]
    # +0 and -0 differ in bits but not in value: an exact sum of zeros may come back with either sign
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    if not bad.any():
        return []
    idx = tuple(int(v) for v in np.argwhere(bad)[0])
    return [f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {idx}: got {got[idx]!r}, want {want[idx]!r}"]


# ----------------------------------------------------------------------------------------------------------- the dispatch
def _cdiv(a, b):
    return (a + b - 1) // b


def narrow_conv_split(M, N, K, mode, deterministic, slab, slab_cap, flags=0, c_aligned=True):
    """narrow_conv_split of gemm.hip: (split_k, atomic) it sets for a conv forward / data gradient, or None."""
    if mode != MODE_F32X3 or (deterministic and not slab) or flags:
        return None
    if N <= 64 or N > 128 or (N & 3) or M < 256 or not c_aligned:
        return None
    tiles = _cdiv(M, 256)
    if tiles >= 192:
        return None
    sk = 2
    while sk <= 8:
        if K % (16 * sk):
            return None
        if (K // sk // 16) * TAPS < 24:
            return None
        if tiles * sk >= 192:
            if slab:
                return None if sk > slab_cap else (sk, False)
            return (sk, True)
        sk *= 2
    return None


def launch_gemm(M, N, K, a_kc, b_kc, mode, *, epi=EPI_STORE, act=ACT_NONE, split_k=1, slab=False, slab_cap=0, batch=1,
                tap_mode=0, a16=False, b16=False, c16=False, bias=False, bn=False, bn_groups=1, bn_nseg=1,
                deterministic=False, lda=None, ldb=None, ldc=None, c_aligned=True, c_tap_stride=0, b_tap_stride=0):
    """launch_gemm of gemm.hip restated (the product build: every development knob at its constant).  None = DVAE_EINVAL;
    otherwise the fields of the launch: which kernel, its template arguments, the k-split, the grid and the tile map."""
    taps = TAPS if tap_mode else 1
    lda = lda if lda is not None else (K if a_kc else M)
    ldb = ldb if ldb is not None else (K if b_kc else N)
    ldc = ldc if ldc is not None else N
    if (a16 or b16 or c16) and mode != MODE_BF16:
        return None
    if c16 and (epi != EPI_STORE or split_k > 1):
        return None
    if a16 and ((lda & 7) or ((K & 7) if a_kc else (M & 7))):
        return None
    if b16 and ((ldb & 7) or ((K & 7) if b_kc else (N & 7))):
        return None
    if b16 and tap_mode == 1 and (b_tap_stride & 7):
        return None
    if M <= 0 or N <= 0 or K <= 0 or (lda & 3) or (ldb & 3) or ((a_kc or b_kc) and (K & 3)):
        return None
    if (not a_kc and (M & 3)) or (not b_kc and (N & 3)):
        return None
    if split_k < 1 or (deterministic and not slab):
        split_k = 1
    if slab:
        if slab_cap < 0 or c16 or act != ACT_NONE or epi not in (EPI_STORE, EPI_ACCUM):
            return None
        if split_k > slab_cap:
            split_k = slab_cap if slab_cap > 0 else 1
    elif split_k > 1 and (epi != EPI_ATOMIC or act != ACT_NONE):
        return None
    splittable = slab or epi == EPI_ATOMIC
    max_sk = (slab_cap if slab_cap > 0 else 1) if slab else (1 << 30)
    if epi != EPI_STORE and act != ACT_NONE:
        return None
    kps = _cdiv(K, split_k)
    bk = 32 if ((kps % 32 == 0 and kps >= 64) or (split_k > 1 and kps >= 512)) else 16
    bf = mode == MODE_BF16
    if bf:
        bk = 32
    if mode == MODE_F32X3:
        bk = 16
    kps = _cdiv(kps, bk) * bk
    split_k = _cdiv(K, kps)
    if batch > 1 and (tap_mode != 0 or bias or bn or batch > 4 or c16):
        return None
    zt = taps if tap_mode == 2 else 1
    zdim = split_k * zt
    a_bytes = (M if a_kc else K) * lda * 4
    b_bytes = (N if b_kc else K) * ldb * 4 * (taps if tap_mode == 1 else 1)
    c_ok = N % 4 == 0 and ldc % 4 == 0 and c_aligned and c_tap_stride % 4 == 0
    tall = False
    if mode == MODE_F32X3 and K % 16 == 0 and a_bytes < (1 << 30) and b_bytes < (1 << 30) and c_ok and M >= 256 and N > 64 \
            and batch <= 1:
        t2 = _cdiv(M, 256) * _cdiv(N, 128)
        half = _cdiv(kps // 2, bk) * bk
        if t2 * zdim < 192 and split_k > 1 and splittable and kps >= 1024 and _cdiv(K, half) <= max_sk:
            kps = half
            split_k = _cdiv(K, kps)
            zdim = split_k * zt
        tall = t2 * zdim >= 192 and (kps // 16) * (taps if tap_mode == 1 else 1) >= 8
    tall16 = False
    if bf and batch <= 1 and a16 and b16 and not c16 and M >= 256 and N > 64 and K % 64 == 0 and c_ok and \
            a_bytes < (1 << 31) and b_bytes < (1 << 31):
        kps64 = _cdiv(kps, 64) * 64
        sk64 = _cdiv(K, kps64)
        t2 = _cdiv(M, 256) * _cdiv(N, 128)
        half = _cdiv(kps64 // 2, 64) * 64
        if t2 * sk64 * zt < 192 and split_k > 1 and splittable and kps64 >= 1024 and _cdiv(K, half) <= max_sk:
            kps64 = half
            sk64 = _cdiv(K, kps64)
        if t2 * sk64 * zt >= 192 and (kps64 // 64) * (taps if tap_mode == 1 else 1) >= 8:
            tall16, kps, split_k, zdim = True, kps64, sk64, sk64 * zt
    t256 = False
    if bf and batch <= 1 and a16 and b16 and not c16 and a_kc == b_kc and M >= 256 and N >= 256 and K % 64 == 0 and \
            N % 8 == 0 and M % 8 == 0 and ldc % 4 == 0 and c_aligned and c_tap_stride % 4 == 0 and \
            a_bytes < (1 << 31) and b_bytes < (1 << 31):
        tz = _cdiv(M, 256) * _cdiv(N, 256) * zt
        sk = 1
        if split_k > 1 and slab:
            sk = max(256 // tz, 1)
        sk = min(sk, max_sk)
        kps256 = _cdiv(_cdiv(K, sk), 64) * 64
        if kps256 < 512 and sk > 1:
            kps256 = 512
        sk = _cdiv(K, kps256)
        iters = (kps256 // 64) * (taps if tap_mode == 1 else 1)
        epi_ok = epi != EPI_ATOMIC and act != ACT_TANH and (split_k == 1 or slab) and (a_kc or tz >= 20)
        if epi_ok and tz * sk >= 224 and iters >= 8:
            t256, tall16, kps, split_k, zdim = True, False, kps256, sk, sk * zt
    tiles256 = _cdiv(M, 256) * _cdiv(N, 256) * zdim
    big = bk == 32 and tiles256 >= 512 and N >= 256 and M >= 256 and tap_mode == 0 and batch <= 1 and mode == MODE_F32
    bm = 256 if (big or tall or tall16 or t256) else 128
    tiles_m = _cdiv(M, bm)
    tiles128 = tiles_m * _cdiv(N, 128) * zdim
    narrow = not (big or tall or tall16 or t256) and tiles128 < 256 and N > 32
    bn_ = 256 if (big or t256) else (64 if narrow else 128)
    tiles_n = _cdiv(N, bn_)
    xcd_map = tiles_m % 8 == 0 and not big
    per, conc = tiles_m >> 3, (32 if (tall or tall16 or t256) else 64)
    gn = max(d for d in range(1, 9) if tiles_n % d == 0)
    gm = max([d for d in range(1, conc // gn + 1) if d <= per and per % d == 0] or [1])
    if bn and (not a_kc or not b_kc or big or split_k != 1 or epi != EPI_STORE or act != ACT_NONE):
        return None
    bn_uniform = bool(bn) and bn_groups >= 1 and (bn_nseg // bn_groups) % 64 == 0 and bn_nseg % bn_groups == 0
    kernel = "bf16_256" if t256 else "bf16_tall" if tall16 else "x3_tall" if tall else "f32"
    wg = 4 if big else 3 if t256 else 1 if (tall or tall16) else 2
    d = dict(kernel=kernel, A_KC=int(a_kc), B_KC=int(b_kc), NTW=1 if narrow else 2, BK=bk, WG=wg, MODE=mode, BNS=int(bool(bn)),
             A16=int(a16), B16=int(b16), tap_mode=tap_mode, BNU=int(bn_uniform and kernel != "f32"),
             split_k=split_k, k_per_split=kps, bm=bm, bn=bn_, tiles_m=tiles_m, tiles_n=tiles_n, zdim=zdim * max(batch, 1),
             narrow=narrow, tall=tall, tall16=tall16, t256=t256, big=big, xcd_map=int(xcd_map), map_gm=gm, map_gn=gn,
             map_nstr=tiles_n // gn, c_vec=int(not c16 and c_ok), to_slab=bool(slab and split_k > 1))
    d["tag"] = encode_tag(d)
    return d


TAG_FIELDS = ("kernel", "A_KC", "B_KC", "NTW", "BK", "WG", "MODE", "BNS", "A16", "B16", "tap_mode")


def encode_tag(d):
    return (d["A_KC"] | d["B_KC"] << 1 | d["NTW"] << 2 | d["BK"] << 4 | d["WG"] << 10 | d["MODE"] << 13 | d["tap_mode"] << 15 |
            d["A16"] << 17 | d["B16"] << 18 | d["BNS"] << 19)


def decode_tag(t):
    """The fields of a launch tag (dvae_prof_collect_tags): launch_gemm's own record of the instantiation it started."""
    wg, mode = (t >> 10) & 7, (t >> 13) & 3
    kernel = "bf16_256" if wg == 3 else ("bf16_tall" if mode == MODE_BF16 else "x3_tall") if wg == 1 else "f32"
    return dict(kernel=kernel, A_KC=t & 1, B_KC=(t >> 1) & 1, NTW=(t >> 2) & 3, BK=(t >> 4) & 63, WG=wg, MODE=mode,
                BNS=(t >> 19) & 1, A16=(t >> 17) & 1, B16=(t >> 18) & 1, tap_mode=(t >> 15) & 3)


def tile_of(bid, d):
    """gemm_tile_of of gemm_common.h: workgroup blockIdx.x -> (tile_m, tile_n)."""
    if d["xcd_map"]:
        per, x, q = d["tiles_m"] >> 3, bid & 7, bid >> 3
        blk = d["map_gm"] * d["map_gn"]
        rnd, r = divmod(q, blk)
        mg, st = divmod(rnd, d["map_nstr"])
        rm = r // d["map_gn"]
        return x * per + mg * d["map_gm"] + rm, st * d["map_gn"] + (r - rm * d["map_gn"])
    return bid % d["tiles_m"], bid // d["tiles_m"]


def expected_kernel(c):
    """The launch a case must reach: launch_gemm (+ narrow_conv_split) restated for the case's entry point."""
    mode = MODES[c.mode]
    kw = dict(a16=c.a16, b16=c.b16, c16=c.c16, deterministic=c.deterministic)
    slab = c.slab_cap is not None
    if not is_conv(c):
        cap = (c.slab_cap // c.batch if c.batch > 1 else c.slab_cap) if slab else 0
        return launch_gemm(c.M, c.N, c.K, c.a_kc, c.b_kc, mode, epi=c.epi, act=c.act, split_k=c.split, slab=slab, slab_cap=cap,
                           batch=c.batch, bias=c.bias, ldc=c.N + c.ldc_pad, c_aligned=c.c_off % 4 == 0, **kw)
    if is_wgrad(c):      # M = Cout, N = Cin, K = R, both operands row-contiguous
        return launch_gemm(c.M, c.N, c.K, False, False, mode, epi=c.epi, split_k=c.split, slab=slab, slab_cap=c.slab_cap or 0,
                           tap_mode=2, c_tap_stride=c.M * c.N, **kw)
    split, epi = 1, EPI_STORE
    if c.entry != "conv_fwd_stats":
        flags = (A_BF16 if c.a16 else 0) | (B_BF16 if c.b16 else 0)
        ns = narrow_conv_split(c.M, c.N, c.K, mode, c.deterministic, slab, c.slab_cap or 0, flags)
        if ns:
            split, epi = ns[0], (EPI_ATOMIC if ns[1] else EPI_STORE)
    slab = slab and split > 1
    return launch_gemm(c.M, c.N, c.K, True, True, mode, epi=epi, split_k=split, slab=slab, slab_cap=c.slab_cap or 0,
                       tap_mode=1, bias=c.bias, bn=c.entry == "conv_fwd_stats", bn_groups=c.G or 1, bn_nseg=c.nseg,
                       b_tap_stride=c.N * c.K, **kw)


def instantiation(d):
    """The kernel template instantiation behind a launch (what launch_variant / launch_bns / launch_gemm pick)."""
    if d["kernel"] == "f32":
        return ("gemm_f32_kernel", d["A_KC"], d["B_KC"], d["NTW"], d["BK"], d["WG"], d["MODE"], d["BNS"], d["A16"], d["B16"])
    if d["kernel"] == "bf16_256":
        return ("gemm_bf16_256_kernel", d["A_KC"], d["B_KC"], d["BNS"], d["BNU"])
    name = "gemm_x3_tall_kernel" if d["kernel"] == "x3_tall" else "gemm_bf16_tall_kernel"
    return (name, d["A_KC"], d["B_KC"], d["BNS"], d["BNU"])


def all_instantiations():
    """Every instantiation launch_gemm, launch_variant and launch_bns can start in the product build."""
    out = set()
    lay = [(a, b) for a in (0, 1) for b in (0, 1)]
    for a, b in lay:
        for ntw in (1, 2):
            for bk in (16, 32):
                out.add(("gemm_f32_kernel", a, b, ntw, bk, 2, MODE_F32, 0, 0, 0))
            out.add(("gemm_f32_kernel", a, b, ntw, 16, 2, MODE_F32X3, 0, 0, 0))
            for a16 in (0, 1):
                for b16 in (0, 1):
                    out.add(("gemm_f32_kernel", a, b, ntw, 32, 2, MODE_BF16, 0, a16, b16))
        out.add(("gemm_f32_kernel", a, b, 2, 32, 4, MODE_F32, 0, 0, 0))
        out.add(("gemm_x3_tall_kernel", a, b, 0, 0))
        out.add(("gemm_bf16_tall_kernel", a, b, 0, 0))
    for ntw in (1, 2):          # launch_bns: k-contiguous operands only
        for bk in (16, 32):
            out.add(("gemm_f32_kernel", 1, 1, ntw, bk, 2, MODE_F32, 1, 0, 0))
        out.add(("gemm_f32_kernel", 1, 1, ntw, 16, 2, MODE_F32X3, 1, 0, 0))
        for a16 in (0, 1):
            for b16 in (0, 1):
                out.add(("gemm_f32_kernel", 1, 1, ntw, 32, 2, MODE_BF16, 1, a16, b16))
    for name in ("gemm_x3_tall_kernel", "gemm_bf16_tall_kernel", "gemm_bf16_256_kernel"):
        out.add((name, 1, 1, 1, 0))
        out.add((name, 1, 1, 1, 1))
    out.add(("gemm_bf16_256_kernel", 1, 1, 0, 0))
    out.add(("gemm_bf16_256_kernel", 0, 0, 0, 0))
    return out


# ----------------------------------------------------------------------------------------------------------- CASES
LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]
_L = {(True, True): "kk", (True, False): "kr", (False, True): "rk", (False, False): "rr"}


def _mk():
    cs = []

    def add(name, **kw):
        # every case runs every class that applies to its arithmetic: E3 needs two bf16 terms per operand, so the bf16 mode
        # (one term) has none; nothing else is left out
        kw["classes"] = ("E1", "E2", "R") if kw.get("mode") == "bf16" else ("E1", "E2", "E3", "R")
        cs.append(Case(name=name, **kw))

    # ---- the 128 x 64 NTW tile: every layout x NTW x k-tile x arithmetic, ragged M / N where the layout allows
    for a_kc, b_kc in LAYOUTS:
        ll = _L[(a_kc, b_kc)]
        for ntw in (2, 1):
            M = 130 if a_kc else 132
            N = {2: 30 if b_kc else 32, 1: 70 if b_kc else 72}[ntw]
            for mode, K in (("fp32", 48), ("fp32", 64), ("fp32x3", 80)):
                add(f"tile-{mode}-{ll}-ntw{ntw}-K{K}", M=M, N=N, K=K, a_kc=a_kc, b_kc=b_kc, mode=mode, bias=True,
                    act=ACT_RELU if ntw == 1 else ACT_NONE,
                    reach=dict(kernel="f32", NTW=ntw, BK=32 if K == 64 else 16, WG=2))
            for a16 in (False, True):
                for b16 in (False, True):
                    M8 = 136 if (a16 and not a_kc) else M
                    N8 = {2: 32, 1: 72}[ntw] if (b16 and not b_kc) else N
                    add(f"tile-bf16-{ll}-ntw{ntw}-a16{int(a16)}-b16{int(b16)}", M=M8, N=N8, K=72 if not (a16 or b16) else 80,
                        a_kc=a_kc, b_kc=b_kc, mode="bf16", a16=a16, b16=b16, bias=True,
                        reach=dict(kernel="f32", NTW=ntw, BK=32, WG=2, A16=int(a16), B16=int(b16)))
    add("tiny-7x4x20", M=7, N=4, K=20, reach=dict(kernel="f32", NTW=2))
    add("rr-K6", M=8, N=2048, K=6, a_kc=False, b_kc=False, reach=dict(kernel="f32", NTW=1))
    add("ntw1-130x260x516", M=130, N=260, K=516, bias=True, reach=dict(kernel="f32", NTW=1))
    add("ntw2-by-count", M=2048, N=256, K=512, epi=EPI_ATOMIC, split=8, bias=True,
        reach=dict(kernel="f32", NTW=2))
    add("fp32-split-bk32-ragged", M=132, N=72, K=2096, mode="fp32", a_kc=False, b_kc=False, epi=EPI_ATOMIC, split=4,
        reach=dict(kernel="f32", BK=32, k_per_split=544, split_k=4))
    # ---- epilogues, in each arithmetic
    for mode in ("fp32", "fp32x3", "bf16"):
        sh = dict(M=200, N=72, K=80, mode=mode)
        add(f"epi-{mode}-store", **sh)
        add(f"epi-{mode}-bias-tanh", bias=True, act=ACT_TANH, **sh)
        add(f"epi-{mode}-bias-relu-rr", bias=True, act=ACT_RELU, a_kc=False, b_kc=False, **sh)
        add(f"epi-{mode}-accum", epi=EPI_ACCUM, bias=True, **sh)
        add(f"epi-{mode}-accum-novec", epi=EPI_ACCUM, M=200, N=70, K=80, mode=mode)
        add(f"epi-{mode}-atomic-bias-split3", epi=EPI_ATOMIC, bias=True, split=3, M=130, N=260, K=516, mode=mode,
            reach=dict(split_k=3))
        add(f"epi-{mode}-atomic-one-tile-splits", epi=EPI_ATOMIC, bias=True, split=5, M=200, N=72, K=80, mode=mode,
            reach=dict(split_k=3 if mode == "bf16" else 5))
        add(f"epi-{mode}-ldc-pad", bias=True, ldc_pad=12, **sh)
        add(f"epi-{mode}-ldc-pad-odd", bias=True, ldc_pad=3, **sh)
        add(f"epi-{mode}-c-unaligned", bias=True, c_off=1, **sh)
    add("epi-bf16-c16", M=200, N=72, K=80, mode="bf16", c16=True, bias=True, act=ACT_RELU)
    add("epi-bf16-c16-a16-b16", M=200, N=72, K=80, mode="bf16", a16=True, b16=True, c16=True)
    # ---- batched launches: 2, 3, 4 products, B shared or not, unsplit and split
    for nb in (2, 3, 4):
        add(f"batched{nb}-accum", entry="batched", batch=nb, M=132, N=72, K=80, a_kc=False, b_kc=False, epi=EPI_ACCUM,
            shared_b=nb == 3)
        add(f"batched{nb}-atomic-split", entry="batched", batch=nb, M=132, N=72, K=516, a_kc=False, b_kc=False, epi=EPI_ATOMIC,
            split=3, shared_b=nb != 3, reach=dict(split_k=3))
        add(f"batched{nb}-slabs", entry="batched_slabs", batch=nb, use_fold=nb != 3, M=132, N=72, K=516, a_kc=False, b_kc=False, epi=EPI_ACCUM,
            split=4, slab_cap=4 * nb, shared_b=nb == 2, reach=dict(split_k=4))
    add("batched2-kk-store", entry="batched", batch=2, M=130, N=70, K=80, epi=EPI_STORE, mode="fp32")
    add("batched3-slabs-clamped", entry="batched_slabs", batch=3, M=132, N=72, K=516, a_kc=False, b_kc=False, epi=EPI_STORE,
        split=4, slab_cap=8, reach=dict(split_k=2))
    # ---- slabs: the clamp, no slabs, ACCUM and STORE, bias on split 0; use_fold: summed by dvae_slab_fold (ACCUM only: it
    # adds to C), the others by dvae_slab_sum
    add("slabs-split4", entry="slabs", M=130, N=260, K=516, split=4, slab_cap=16, bias=True, reach=dict(split_k=4))
    add("slabs-clamp", entry="slabs", use_fold=True, M=130, N=260, K=516, split=6, slab_cap=3, epi=EPI_ACCUM, reach=dict(split_k=3))
    add("slabs-cap0", entry="slabs", M=130, N=260, K=516, split=6, slab_cap=0, epi=EPI_ACCUM, bias=True, reach=dict(split_k=1))
    add("slabs-fp32-rr", entry="slabs", use_fold=True, M=132, N=72, K=2096, mode="fp32", a_kc=False, b_kc=False, split=4, slab_cap=16,
        epi=EPI_ACCUM, reach=dict(split_k=4, BK=32))
    add("slabs-bf16", entry="slabs", M=130, N=260, K=516, mode="bf16", split=4, slab_cap=16)
    # ---- the workgroup -> tile map on the device: every tile must hold its own exact block
    for tm in (8, 16, 24):
        for tn in (1, 3, 7, 9, 11):
            add(f"xcd-{tm}x{tn}", M=128 * tm, N=64 * tn, K=32, mode="fp32x3" if tn != 7 else "fp32",
                reach=dict(kernel="f32", NTW=1, xcd_map=1, tiles_m=tm, tiles_n=tn, map_gn={1: 1, 3: 3, 7: 7, 9: 3, 11: 1}[tn]))
    # ---- fp32x3 tall tile (256 x 128)
    for a_kc, b_kc in LAYOUTS:
        add(f"tall-x3-{_L[(a_kc, b_kc)]}", M=6144, N=1024, K=128, a_kc=a_kc, b_kc=b_kc, bias=True, reach=dict(kernel="x3_tall"))
    add("tall-x3-ragged-kk", M=6144 + 40, N=1020, K=128, bias=True, act=ACT_RELU,
        reach=dict(kernel="x3_tall"))
    add("tall-x3-ragged-rr", M=6144 + 40, N=1020, K=128, a_kc=False, b_kc=False, epi=EPI_ACCUM,
        reach=dict(kernel="x3_tall"))
    add("tall-x3-K136-falls-back", M=6144, N=1024, K=136, reach=dict(kernel="f32", NTW=2))
    add("tall-x3-split-atomic", M=1024, N=512, K=1536, epi=EPI_ATOMIC, split=12, bias=True,
        reach=dict(kernel="x3_tall", split_k=12, k_per_split=128))
    add("tall-x3-split-slabs", entry="slabs", use_fold=True, M=1024, N=512, K=1536, a_kc=False, b_kc=False, epi=EPI_ACCUM, split=12,
        slab_cap=24, reach=dict(kernel="x3_tall", split_k=12))
    # (the tall rule halves k_per_split >= 1024 while the grid is under 192 workgroups: 8 splits asked, 16 launched)
    add("tall-x3-split-doubled-atomic", M=1024, N=512, K=8192, epi=EPI_ATOMIC, split=8, bias=True,
        reach=dict(kernel="x3_tall", split_k=16, k_per_split=512))
    add("tall-x3-split-doubled-slabs", entry="slabs", M=1024, N=512, K=8192, epi=EPI_STORE, split=8, slab_cap=16, bias=True, reach=dict(kernel="x3_tall", split_k=16))
    add("tall-x3-split-not-doubled-cap", entry="slabs", M=1024, N=512, K=8192, epi=EPI_STORE, split=8, slab_cap=12, reach=dict(kernel="f32", split_k=8))
    # ---- fp32 16-wave tile (256 x 256)
    add("big-kk", M=8192, N=4096, K=64, mode="fp32", bias=True, reach=dict(kernel="f32", WG=4))
    add("big-rr-ragged", M=8192 + 8, N=4096 + 4, K=64, mode="fp32", a_kc=False, b_kc=False,
        reach=dict(kernel="f32", WG=4))
    add("big-kr-ragged", M=8192 + 8, N=4096 + 4, K=64, mode="fp32", a_kc=True, b_kc=False, act=ACT_RELU, bias=True, reach=dict(kernel="f32", WG=4))
    add("big-rk", M=8192, N=4096, K=64, mode="fp32", a_kc=False, b_kc=True, epi=EPI_ACCUM,
        reach=dict(kernel="f32", WG=4))
    add("big-atomic-split8", M=2048, N=2048, K=512, mode="fp32", epi=EPI_ATOMIC, split=8, bias=True,
        reach=dict(kernel="f32", WG=4, split_k=8))
    # ---- bf16 tall (both operands bf16 in memory) and the 256 x 256 LDS-DMA kernel at its threshold
    for a_kc, b_kc in LAYOUTS:
        add(f"tall16-{_L[(a_kc, b_kc)]}", M=6144, N=1024, K=512, a_kc=a_kc, b_kc=b_kc, mode="bf16", a16=True, b16=True,
            bias=a_kc, reach=dict(kernel="bf16_tall"))
    add("g256-kk", M=4096, N=3584, K=512, mode="bf16", a16=True, b16=True, bias=True, act=ACT_RELU,
        reach=dict(kernel="bf16_256"))
    add("g256-rr", M=4096, N=3584, K=512, a_kc=False, b_kc=False, mode="bf16", a16=True, b16=True,
        reach=dict(kernel="bf16_256"))
    # ---- Conv1d(k = 5): M = rows R = T nseg (wgrad: M = Cout, N = Cin, K = R), K = input channels of the product
    for nseg in (1, 2, 5):
        for T in (1, 2, 3, 5, 9):
            R = nseg * T
            tag = f"n{nseg}-t{T}"
            add(f"conv-fwd-{tag}", entry="conv_fwd", M=R, N=80, K=80, nseg=nseg, bias=True,
                reach=dict(kernel="f32", tap_mode=1))
            add(f"conv-dgrad-{tag}", entry="conv_dgrad", M=R, N=80, K=80, nseg=nseg,
                mode="fp32" if T == 3 else "fp32x3", reach=dict(kernel="f32", tap_mode=1))
            add(f"conv-wgrad-{tag}", entry="conv_wgrad", M=80, N=80, K=R, nseg=nseg, epi=EPI_ATOMIC, split=1,
                a_kc=False, b_kc=False, reach=dict(kernel="f32", tap_mode=2))
    add("conv-fwd-512-80", entry="conv_fwd", M=45, N=80, K=512, nseg=5, bias=True)
    add("conv-fwd-80-512-bf16", entry="conv_fwd", M=45, N=512, K=80, nseg=5, bias=True, mode="bf16")
    add("conv-fwd-36-20", entry="conv_fwd", M=45, N=20, K=36, nseg=5, bias=True, mode="fp32")
    add("conv-dgrad-512-80", entry="conv_dgrad", M=45, N=80, K=512, nseg=5)
    add("conv-dgrad-20-36", entry="conv_dgrad", M=45, N=36, K=20, nseg=5, mode="fp32")
    add("conv-wgrad-512-80-split", entry="conv_wgrad", M=512, N=80, K=645, nseg=5, epi=EPI_ATOMIC, split=3, a_kc=False,
        b_kc=False, reach=dict(split_k=3, k_per_split=224))
    add("conv-wgrad-36-20-split-fp32", entry="conv_wgrad", M=20, N=36, K=645, nseg=5, epi=EPI_ATOMIC, split=4, a_kc=False,
        b_kc=False, mode="fp32", reach=dict(split_k=4, k_per_split=176))
    add("conv-wgrad-slabs", entry="conv_wgrad_slabs", use_fold=True, M=80, N=512, K=645, nseg=5, epi=EPI_ACCUM, split=3, slab_cap=8,
        a_kc=False, b_kc=False, reach=dict(split_k=3))
    add("conv-wgrad-slabs-unsplit", entry="conv_wgrad_slabs", M=80, N=80, K=45, nseg=5, epi=EPI_STORE, split=1, slab_cap=8,
        a_kc=False, b_kc=False, reach=dict(split_k=1))
    # narrow_conv_split: 80 output columns, the smallest R with tiles x 2 >= 192 at K = 160 (steps = 25)
    ncs = dict(M=95 * 256 + 1, N=80, K=160, nseg=3, bias=True)
    add("conv-fwd-narrow-split", entry="conv_fwd", reach=dict(kernel="x3_tall", split_k=2), **ncs)
    add("conv-fwd-narrow-deterministic", entry="conv_fwd", deterministic=True, reach=dict(kernel="f32", split_k=1),
        **ncs)
    add("conv-dgrad-narrow-split", entry="conv_dgrad", reach=dict(kernel="x3_tall", split_k=2), **{**ncs, "bias": False})
    add("conv-fwd-narrow-slabs", entry="conv_fwd_slabs", slab_cap=4, reach=dict(kernel="x3_tall", split_k=2), **ncs)
    add("conv-dgrad-narrow-slabs", entry="conv_dgrad_slabs", slab_cap=4, reach=dict(kernel="x3_tall", split_k=2),
        **{**ncs, "bias": False})
    add("conv-fwd-slabs-cap1", entry="conv_fwd_slabs", slab_cap=1, reach=dict(split_k=1), **ncs)
    # conv forward with the BatchNorm statistics epilogue: G = 1 and 2, uniform and general chunks
    for mode, K in (("fp32", 80), ("fp32", 64), ("fp32x3", 80), ("bf16", 80)):
        for N in (80, 32):
            add(f"conv-stats-{mode}-K{K}-N{N}", entry="conv_fwd_stats", M=5 * 36, N=N, K=K, nseg=36, G=2 if N == 80 else 1,
                bias=True, mode=mode, reach=dict(kernel="f32", BNS=1, NTW=1 if N == 80 else 2))
    for a16, b16 in ((True, False), (False, True), (True, True)):
        for N in (80, 32):
            add(f"conv-stats-bf16-a16{int(a16)}-b16{int(b16)}-N{N}", entry="conv_fwd_stats", M=5 * 36, N=N, K=80, nseg=36,
                G=2 if N == 80 else 1, bias=True, mode="bf16", a16=a16, b16=b16,
                reach=dict(kernel="f32", BNS=1, NTW=1 if N == 80 else 2, A16=int(a16), B16=int(b16)))
    add("conv-stats-uniform", entry="conv_fwd_stats", M=3 * 128, N=80, K=80, nseg=128, G=2, bias=True,
        reach=dict(kernel="f32", BNS=1))
    add("conv-stats-tall-uniform", entry="conv_fwd_stats", M=384 * 128, N=128, K=32, nseg=128, G=2, bias=True,
        reach=dict(kernel="x3_tall", BNS=1, BNU=1))
    add("conv-stats-tall-general", entry="conv_fwd_stats", M=512 * 96, N=128, K=32, nseg=96, G=2, bias=True,
        reach=dict(kernel="x3_tall", BNS=1, BNU=0))
    for nseg, bnu in ((128, 1), (96, 0)):
        add(f"conv-stats-tall16-bnu{bnu}", entry="conv_fwd_stats", M=49152, N=128, K=128, nseg=nseg, G=2, bias=True, mode="bf16",
            a16=True, b16=True, reach=dict(kernel="bf16_tall", BNS=1, BNU=bnu))
        add(f"conv-stats-g256-bnu{bnu}", entry="conv_fwd_stats", M=57344 if bnu else 57600, N=256, K=128, nseg=nseg, G=2, bias=True,
            mode="bf16", a16=True, b16=True, reach=dict(kernel="bf16_256", BNS=1, BNU=bnu))
    return cs


CASES = _mk()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

# Instantiations of `all_instantiations` that no case reaches, with the reason each cannot be: none.  (The development
# build's knobs can force further combinations — a tall tile below its threshold, the 16 x 16 shape of gemm256.hip — which
# the product library never launches.)
UNREACHED = {}


# ----------------------------------------------------------------------------------------------------------- inputs, verdicts
Inputs = collections.namedtuple("Inputs", "cls role r a b bias base")      # a, b: generated operands (lists when batched)


def gen_dims(c):
    """Shapes of the GENERATED operands: conv forward / data gradient: a = activation rows [R, C], b = [5 C, Nout]."""
    if is_conv(c) and not is_wgrad(c):
        return (c.M, c.K), (TAPS * c.K, c.N)
    return (c.M, c.K), (c.K, c.N)


def roles_of(c, cls):
    """Which operand is the selected (E1) / sparse (E3) one.  A conv forward / data gradient sums its five taps: only a
    selected / sparse WEIGHT keeps one (eight) term(s) per output."""
    if cls not in ("E1", "E3"):
        return (None,)
    return ("B",) if (is_conv(c) and not is_wgrad(c)) else ("A", "B")


def offsets_of(c, cls, d):
    """The offsets r a case runs E1 / E3 at (d: its launch, `expected_kernel`): see `e1_offsets`."""
    if cls not in ("E1", "E3"):
        return (0,)
    M, N, K = logical_dims(c)
    if is_conv(c) and not is_wgrad(c):      # k(j) walks the 5 C taps with the stride C + 1: two offsets, a tap and a bit apart
        return (0, 2 * c.K + 1)
    return e1_offsets(K, min(M, N), d["k_per_split"], d["BK"])


def make_inputs(c, cls, role=None, r=0):
    (Ma, Ka), (Kb, Nb) = gen_dims(c)
    M, N, K = logical_dims(c)
    stride = c.K + 1 if (is_conv(c) and not is_wgrad(c)) else 1
    nout = n_outputs(c)
    want_base = has_base(c)
    As, Bs, bias, bases = [], [], None, None
    cat = is_conv(c) and not is_wgrad(c)         # a = the activation rows [R, C]; b is generated against the 5 C taps
    amp = 1 if c.entry == "conv_fwd_stats" else 15
    Mg = 1 if cat else Ma                        # (the a generated beside such a b is not used)
    for i in range(c.batch):
        key = f"{c.name}/{i}"
        if cls == "E1":
            a, b = e1(key, Mg, Nb, Kb, role, r, stride)
            bi = None
        elif cls == "E3":
            a, b = e3(key, Mg, Nb, Kb, role, r, stride)
            bi = None
        elif cls == "E2":
            a, b, bi, _ = e2(key, Mg, Nb, Kb, c.bias, False, amp)
        else:
            a, b, bi, _ = rclass(key, Mg, Nb, Kb, c.bias, False)
        if cat:
            rs = rng_of(cls, key, "activation", r)
            a = {"E1": lambda: full_sig(rs, (Ma, Ka), -20, 20),
                 "E3": lambda: ((2 * rs.integers(0, 512, (Ma, Ka)) + 1) * (rs.integers(0, 2, (Ma, Ka)) * 2 - 1)).astype(F),
                 "E2": lambda: rs.integers(-amp, amp + 1, (Ma, Ka)).astype(F),
                 "R": lambda: full_sig(rs, (Ma, Ka), -1, 1)}[cls]()
        if i > 0 and c.shared_b:
            b = Bs[0]
        As.append(a)
        Bs.append(b)
        bias = bi if i == 0 else bias
    if want_base:
        rs = rng_of("base", c.name, cls)
        if cls == "E2":
            bases = [rs.integers(-100000, 100001, (M, N)).astype(F) for _ in range(nout)]
        elif cls == "R":
            zr, sr, sc = r_blocks(M, N)
            rowsc, colsc = np.ones((M, 1), F), np.ones(N, F)
            rowsc[sr], colsc[sc] = 2.0 ** -12, 2.0 ** 12
            bases = [full_sig(rs, (M, N), -1, 3) * rowsc * colsc for _ in range(nout)]
        else:       # E1 / E3: the result is bit-exact only onto a base of zeros
            bases = [np.zeros((M, N), F) for _ in range(nout)]
    if c.batch > 1:
        return Inputs(cls, role, r, As, Bs, bias, bases)
    return Inputs(cls, role, r, As[0], Bs[0], bias, bases)


def iter_inputs(c, d):
    for cls in c.classes:
        for role in roles_of(c, cls):
            for r in offsets_of(c, cls, d):
                yield make_inputs(c, cls, role, r)


def family_of(d):
    return {"f32": {2: "128x64NTW", 4: "fp32 256x256"}.get(d["WG"], "?"), "x3_tall": "fp32x3 tall", "bf16_tall": "bf16 tall",
            "bf16_256": "bf16 256x256"}[d["kernel"]] + {MODE_F32: " fp32", MODE_BF16: " bf16", MODE_F32X3: " fp32x3"}[d["MODE"]]


def judge(c, d, inp, outs, rho_cache=None, worst=None):
    """Failures of the outputs `outs` (one fp32 [M, N] per logical product) of a case on inputs `inp`."""
    fails = []
    prods = products(c, inp.a, inp.b)
    big = logical_dims(c)[0] * logical_dims(c)[1] * logical_dims(c)[2] > (1 << 28)
    for i, ((a, b), got) in enumerate(zip(prods, outs)):
        base = None if inp.base is None else inp.base[i]
        if inp.cls != "R":
            want = expected_exact(c, a, b, inp.bias, base, big)
            what = f"{inp.cls} role {inp.role} r {inp.r} output {i}"
            if c.act == ACT_TANH:       # exact pre-activation, the device's tanhf on top of it
                over = np.abs(np.asarray(got, F64) - np.tanh(want_u(c, a, b, inp.bias, big))) > \
                    _tanhf_roundings() * EPS32 * np.abs(want.astype(F64)) + BF16_REL * np.abs(want) * c.c16
                f = [f"{what}: {int(over.sum())} elements beyond the tanhf bound"] if over.any() else []
            else:
                f = exact_check(np.asarray(got, F), want, what)
            fails += f
            if worst is not None:
                k = (family_of(d), inp.cls)
                worst[k] = max(worst.get(k, 0.0), 1.0 if f else 0.0)
            continue
        kps = d["k_per_split"] * (TAPS if is_conv(c) and not is_wgrad(c) else 1)
        key = (c.name, i)
        if rho_cache is not None and key in rho_cache:
            rho = rho_cache[key]
        else:
            rho = rho_of(c, a, b, inp.bias, base, kps, d["bm"], d["bn"])
            if rho_cache is not None:
                rho_cache[key] = rho
        f, w, wr = r_check(c, got, a, b, inp.bias, base, d["split_k"], *rho)
        fails += [f"R output {i}: {x}" for x in f]
        if worst is not None:
            for k, v in (((family_of(d), "R max"), w), ((family_of(d), "R rms"), wr)):
                worst[k] = max(worst.get(k, 0.0), v)
    return fails
