"""The float64 reference of the latent, loss, reduction, activation and layout kernels of csrc/elem.hip and the rounding
bounds one launch is held to.  Not a test module: tests/test_elem_ref.py proves the reference against torch float64 autograd
of the reference model's formulas (model/disentangled_vae.py:250-279 forward, :310-327 loss_functionGVAE2;
model/variational_base_vae.py:281-301, 335-348 conversion) and the bounds against an fp32 restatement on the CPU,
tests/test_hip_elem.py holds the kernels to both.  The formulas are the model's, the bounds are derived below, neither
follows what some code computes.

Notation as in tests/bn_ref.py: eps32 = 2^-24 one fp32 rounding, eps64 = 2^-53, g(k) = k eps32 / (1 - k eps32) k roundings
compounded (k need not be an integer), FLOOR = 2^-126.  X = EXPF_ROUNDINGS: the device's expf(x) lies within X eps32 exp(x)
of exp(x) (measured, see EXPF_MEASURED).  E = exp(argument) in float64.  Every bound is a count of roundings times a sum
of absolute values of what the launch READ, never a fraction of a maximum.  A fused multiply-add only removes a rounding.

Bit for bit, no bound
    q_mu / q_lv on the style columns: 0.5f * (a + b), one rounding of the sum, the halving exact: the fp32 numpy statement
    must give the same bits.  s_mu / s_lv are rows [0, Bh) of them.  The content columns of q_mu / q_lv are copies.  dstyle of
    rows >= Bh is +0.0 (the x2 style head is detached).  Every move (mel_to_frames fp32, frames_to_mel, permute_102,
    transpose, conv_pack_w / _wt, gather_crop, mel_to_chunks, chunks_to_mel) moves bits; the bf16 mel_to_frames stores the
    round-to-nearest-even bf16.  conv_unpack_add_w is one fp32 addition.  slab_sum / slab_fold: v + slab 0 + slab 1 + ...
    are plain fp32 additions in that order, nothing to contract: a sequential fp32 numpy sum gives the same bits, and ReLU
    of it is exact (-0.0 and below give +0.0).  act_fwd / act_bwd with act none / ReLU: a select, or a product with 0.f or 1.f.
    The L1 gradient: 0.f where x == recon, else -w or +w with one w for the whole tensor.
z = eps expf(0.5 lv) + mu  (tol_z; lv and mu are the fp32 values above, 0.5 lv is exact)
    expf X roundings of |eps| E, the product one more, the sum one of |z| <= |eps| E + |mu|:
        |z' - z| <= g(X + 2) |eps| E + g(1) |mu|.        Without eps_c (inference) z = mu on the content columns: a copy.
KL term t = 1 + lv - mu^2 - expf(lv)  (tol_term)
    1 + lv, mu^2, their difference and the last difference: every operand passes at most 4 roundings, expf X of its own:
        |t' - t| <= g(4) (1 + |lv| + mu^2 + E) + X eps32 (1 + g(4)) E
    — absolute, not relative to t, which cancels at lv = mu = 0.
kl_fwd: out = (float)(scale * sum_i t_i)
    fp64 accumulation: a thread adds ceil(n / 256) terms, 6 shuffle steps, 3 additions over the waves, the product with the
    scale, 16 more for the reference's own pairwise sum:   a = ceil(n / 256) + 26
        |out' - out| <= |scale| (sum tol_term + a eps64 sum |t|) (1 + eps32) + eps32 |out|.
kl_bwd: G = gout scale (one rounding), dmu = G (-2 mu) (one more), dlv = G (1 - expf(lv)):
        |dmu' - dmu| <= g(2) |dmu|,      |dlv' - dlv| <= |G| (X eps32 (1 + g(3)) E + g(3) |1 - E|)
    (the error of expf is absolute beside a difference that cancels at lv = 0; the subtraction rounds its own result).
l1_sum_fwd, out[1..4] of loss_fwd: out = (float)(scale * sum |x - y|)
    fp32 per thread: every difference rounds once, a trip adds four of them (3 additions) to the accumulator (1), the tail
    one each: K = 4 trips + tail additions at most, trips = ceil(n4 / (blocks 256)), tail = ceil((n & 3) / 256).  Then fp64:
    6 shuffle steps + 3 per workgroup, ceil(blocks / 64) + 6 in the final kernel (ceil(blocks / 256) + 9 in loss_final),
    the scale, the reference's 16:      |out' - out| <= |scale| (g(K + 1) + a eps64) sum |x - y| (1 + eps32) + eps32 |out|.
    The four L1 entries of loss_fwd use the block count and the order of l1_sum_fwd: they must equal it bit for bit.
out[5..7] of loss_fwd: as kl_fwd with nq / ns terms and kl_scale / style_scale.
out[0] = mse_cof (((t1 + t2) + t3) + t4) + kl_cof (t5 + t6) from the device's OWN out[1..6] (inputs, not errors): three sums,
    two products, one sum — no operand passes more than 5 roundings:
        |out0' - out0| <= g(5) (|mse_cof| sum |t_1..4| + |kl_cof| (|t5| + |t6|)).
loss_bwd: w_k = (g0 mse_cof + g[1+k]) l1_scale: a product, a sum (or one FMA), a product:
        |w' - w| <= g(3) (|g0 mse_cof| + |g[1+k]|) |l1_scale|        (not relative to w: the sum may cancel).
    Every non-zero element of d_recon_k is ONE value bit for bit up to sign, that value is within this bound of w_k, the sign
    is -sign(x - recon) decided exactly from the inputs (an fp32 difference is zero only for equal operands: gradual
    underflow), ties give +0.0.  The latent part with W = (g0 kl_cof + g[5 or 6]) kl_scale, or g[7] style_scale, and
    A = the same with absolute values inside:   |dmu' - dmu| <= g(4) A |2 mu|,
        |dlv' - dlv| <= A (X eps32 (1 + g(4)) E + g(4) |1 - E|).
latent_bwd  (absent upstream gradients are zeros: adding one is exact)
    dstyle mu = 0.5 (dz1 + dz2 + dq_mu1 + dq_mu2 + ds_mu): four additions:  tol = 0.5 g(4) (sum of the five absolute values).
    dstyle lv = 0.5 ((dz1 + dz2) eps 0.5 expf(0.5 lv) + dq_lv1 + dq_lv2 + ds_lv): the first term passes its own sum, two
    products (the halving is exact), expf, three additions:  tol = 0.5 (g(6 + X) (|dz1| + |dz2|) |eps| 0.5 E + g(3) (rest)).
    dcontent mu = dz + dq_mu: g(1) (|dz| + |dq_mu|).   dcontent lv = dz eps 0.5 expf(0.5 lv) + dq_lv:
        tol = g(3 + X) |dz eps| 0.5 E + g(1) |dq_lv|;  without eps_c it is 0 + dq_lv, exact.
colsum_add_ws: out += sum_r X[r][c], fp32.  A term passes ceil(rows_pb / 4) additions in its row lane, 2 over the lanes,
    ceil(row blocks / 4) + 2 over the row blocks, 1 into the output:   K = ceil(min(R, rows_pb) / 4) + ceil(nb / 4) + 5,
        |out' - out| <= g(K) (sum_r |X[r][c]| + |old|).
    colsum_add (atomics): one addition per row block into the output in any order: K = ceil(rows / 4) + 2 + nb; under
    dvae_set_deterministic(1) one workgroup walks all rows: K = ceil(R / 4) + 3.  bf16 input widens exactly.
tanh (slab_sum, act_fwd): the argument u is exact (a bit-exact sum, or the input):  |z' - tanh u| <= T eps32 |tanh u|,
    T = bn_ref.TANHF_ROUNDINGS.  act_bwd tanh, du = dz (1 - z^2): bn_ref's formula,
        |du' - du| <= eps32 |dz| (z^2 + |1 - z^2|) + eps32 |du|.
Division (conversion_latents: mean = (sequential fp32 sum of n rows) / (float)n; mul_div: a * (b / c)).  csrc/build.sh passes
    no flag about division.  `hipcc --help` of the installed toolchain documents -fhip-fp32-correctly-rounded-divide-sqrt
    and its -fno- form but not which one holds without a flag, and no other document of the toolchain is installed, so the
    bound takes the worst documented for the faster division: 2.5 ulp (the fdiv limit of the OpenCL C specification, section
    "Relative error as ULPs", which is what the -fno- form relaxes division to) = DIV_ROUNDINGS = 5 roundings of 2^-24.
        conversion_latents: g(n - 1 + 5) sum_r |x_r| / n;      mul_div: g(5 + 1) |a b / c|.
"""
import numpy as np

import bn_ref as B

EPS32, EPS64, FLOOR, g, worst_ratio = B.EPS32, B.EPS64, B.FLOOR, B.g, B.worst_ratio
ACT_NONE, ACT_RELU, ACT_TANH = B.ACT_NONE, B.ACT_RELU, B.ACT_TANH
TANHF_ROUNDINGS = B.TANHF_ROUNDINGS
# Device expf against float64 exp, |expf(x) - exp(x)| / (eps32 exp(x)): measured worst 1.4108 (at x = -42.9318275) over
# 40 000 001 evenly spaced x in [-87, 88] and 2^23 log-spaced |x| in [1e-6, 1] of either sign on the MI355X
# (scripts/probes/expf_sweep.hip).  The sweep is a sample: the bound is twice that.
EXPF_MEASURED = 1.4108
EXPF_ROUNDINGS = 2.0 * EXPF_MEASURED
DIV_ROUNDINGS = 5.0
X = EXPF_ROUNDINGS

F64, F32 = np.float64, np.float32
L1_BLOCKS = 512                # csrc/elem.hip
LOSS_BWD_BLOCKS = 1024         # cap of the L1 part of dvae_loss_bwd's grid
SLAB_FOLD_MAX = 64             # DVAE_SLAB_FOLD_MAX of include/dvae_hip.h
MODEL_S, MODEL_CN = 4, 28      # style and content widths of the model (latent_dim 32)


# ------------------------------------------------------------------ the launch arithmetic, restated
def nblk(n, per=256, cap=2048):
    return int(min(max((n + per - 1) // per, 1), cap))


def l1_launch(n, cap=L1_BLOCKS):
    """blocks, trips of the busiest thread, tail elements of dvae_l1_sum_fwd / dvae_loss_fwd (cap 1024: dvae_loss_bwd)."""
    blocks, n4 = nblk(n // 4 + 1, 256, cap), n >> 2
    return {"blocks": blocks, "trips": -(-n4 // (blocks * 256)), "tail": n & 3}


def colsum_launch(R, C, deterministic=False):
    cb = (C + 255) // 256
    rows_pb = R if deterministic else (1024 if R * cb >= 512 * 1024 else 512)
    return {"cb": cb, "rows_pb": rows_pb, "nb": -(-R // rows_pb), "ragged": C % 4 != 0}


def slab_windows(nslab):
    """(windows of 8, windows of 4, single slabs) slab_add walks."""
    return nslab // 8, (nslab % 8) // 4, nslab % 4


def fold_launches(n_entries):
    return -(-n_entries // SLAB_FOLD_MAX)


# ------------------------------------------------------------------ exp: float64, or an fp32 one pushed to the bound
def exp32(push):
    """An fp32 exp that is wrong by up to EXPF_ROUNDINGS roundings in the direction of `push` (+1 / -1 / 0): float64 exp
    moved by X - 1 roundings, then rounded (the last one)."""
    def f(x):
        with np.errstate(over="ignore"):
            return (np.exp(np.asarray(x, F64)) * (1.0 + push * (X - 1.0) * EPS32)).astype(F32)
    return f


def _z(a, shape, dt):
    return np.zeros(shape, dt) if a is None else np.asarray(a, dt).reshape(shape)


# ------------------------------------------------------------------ the operations (dt = float64: the reference;
# dt = float32 with ex = exp32(push): the kernels' statements, one rounding per operation, in the kernels' order)
def latent_fwd(style, content, eps_c, eps_s, Bh, S, Cn, dt=F64, ex=np.exp):
    """(z, q_mu, q_lv [2Bh, S+Cn], s_mu, s_lv [Bh, S]) of disentangled_vae.py:250-272; eps_c None: z = mu on the content."""
    st, co, h = np.asarray(style, dt).reshape(2 * Bh, 2 * S), np.asarray(content, dt).reshape(2 * Bh, 2 * Cn), dt(0.5)
    s_mu, s_lv = h * (st[:Bh, :S] + st[Bh:, :S]), h * (st[:Bh, S:] + st[Bh:, S:])
    zs = np.asarray(eps_s, dt).reshape(Bh, S) * ex(h * s_lv).astype(dt) + s_mu
    cmu, clv = co[:, :Cn], co[:, Cn:]
    zc = cmu if eps_c is None else np.asarray(eps_c, dt).reshape(2 * Bh, Cn) * ex(h * clv).astype(dt) + cmu
    two = lambda a: np.concatenate([a, a], 0)
    return (np.concatenate([two(zs), zc], 1), np.concatenate([two(s_mu), cmu], 1), np.concatenate([two(s_lv), clv], 1),
            s_mu, s_lv)


def latent_bwd(style, content, eps_c, eps_s, dz, dq_mu, dq_lv, ds_mu, ds_lv, Bh, S, Cn, dt=F64, ex=np.exp, style_half=0.5):
    """(dstyle [2Bh, 2S], dcontent [2Bh, 2Cn]); any of the five upstream gradients may be None."""
    D, h = S + Cn, dt(0.5)
    st, co = np.asarray(style, dt).reshape(2 * Bh, 2 * S), np.asarray(content, dt).reshape(2 * Bh, 2 * Cn)
    dz, dqm, dql = _z(dz, (2 * Bh, D), dt), _z(dq_mu, (2 * Bh, D), dt), _z(dq_lv, (2 * Bh, D), dt)
    dsm, dsl, es = _z(ds_mu, (Bh, S), dt), _z(ds_lv, (Bh, S), dt), np.asarray(eps_s, dt).reshape(Bh, S)
    s_lv = h * (st[:Bh, S:] + st[Bh:, S:])
    gz = dz[:Bh, :S] + dz[Bh:, :S]
    gmu = gz + dqm[:Bh, :S] + dqm[Bh:, :S] + dsm
    glv = gz * es * h * ex(h * s_lv).astype(dt) + dql[:Bh, :S] + dql[Bh:, :S] + dsl
    dstyle, dcontent = np.zeros((2 * Bh, 2 * S), dt), np.zeros((2 * Bh, 2 * Cn), dt)
    dstyle[:Bh, :S], dstyle[:Bh, S:] = dt(style_half) * gmu, dt(style_half) * glv
    dcontent[:, :Cn] = dz[:, S:] + dqm[:, S:]
    first = dt(0) if eps_c is None else dz[:, S:] * np.asarray(eps_c, dt).reshape(2 * Bh, Cn) * h * ex(h * co[:, Cn:]).astype(dt)
    dcontent[:, Cn:] = first + dql[:, S:]
    return dstyle, dcontent


def kl_terms(mu, lv, dt=F64, ex=np.exp, drop_one=False):
    mu, lv = np.asarray(mu, dt).reshape(-1), np.asarray(lv, dt).reshape(-1)
    return (lv if drop_one else dt(1) + lv) - mu * mu - ex(lv).astype(dt)


def kl_fwd(mu, lv, scale, dt=F64, ex=np.exp):
    """scale * sum(1 + lv - mu^2 - exp(lv)); the sum of the terms is float64 on either path."""
    return dt(kl_terms(mu, lv, dt, ex).astype(F64).sum() * float(F32(scale)))


def kl_bwd(mu, lv, gout, scale, dt=F64, ex=np.exp):
    mu, lv = np.asarray(mu, dt).reshape(-1), np.asarray(lv, dt).reshape(-1)
    G = dt(gout) * dt(scale)
    return G * (dt(-2) * mu), G * (dt(1) - ex(lv).astype(dt))


def l1_fwd(x, y, scale):
    return float(np.abs(np.asarray(x, F64) - np.asarray(y, F64)).sum() * float(F32(scale)))


def l1_fwd_f32(x, y, scale, skip_tail=0):
    """l1_partial_kernel + l1_final_kernel: fp32 per thread in the kernel's order, float64 across threads."""
    x, y = np.asarray(x, F32).reshape(-1), np.asarray(y, F32).reshape(-1)
    n = x.size
    la, n4 = l1_launch(n), x.size >> 2
    d = np.abs(x - y)
    q = d[:4 * n4].reshape(n4, 4)
    q = ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]
    T = la["blocks"] * 256
    acc = np.zeros(T, F32)
    for t in range(la["trips"]):
        part = q[t * T:(t + 1) * T]
        acc[:part.size] += part
    tail = d[4 * n4:n - skip_tail]
    acc[:tail.size] += tail
    return F32(acc.astype(F64).sum() * float(F32(scale)))


def l1_bwd(x, y, gout, scale, dt=F64):
    """d/dy of scale sum |x - y| times gout: -G sign(x - y), 0 at a tie."""
    d = np.asarray(x, F64) - np.asarray(y, F64)
    G = dt(gout) * dt(scale)
    return np.where(d > 0, -G, np.where(d < 0, G, dt(0))).astype(dt)


LOSS_KEYS = ("x1", "x2", "recon1", "recon2", "recon1_hat", "recon2_hat", "q1_mu", "q1_lv", "q2_mu", "q2_lv", "s_mu", "s_lv")
SCALE_KEYS = ("l1_scale", "kl_scale", "style_scale", "mse_cof", "kl_cof")


def loss_fwd(d):
    """out[8] of loss_functionGVAE2 (disentangled_vae.py:310-327) in float64; d: the arrays of LOSS_KEYS and the fp32 scalars
    of SCALE_KEYS (l1_scale = 1 / batch_size, kl_scale = -0.5 / rows, style_scale = -1 / batch_size)."""
    t = [l1_fwd(d["x%d" % (1 + (k & 1))], d[LOSS_KEYS[2 + k]], d["l1_scale"]) for k in range(4)]
    t += [float(kl_fwd(d["q1_mu"], d["q1_lv"], d["kl_scale"])), float(kl_fwd(d["q2_mu"], d["q2_lv"], d["kl_scale"])),
          float(kl_fwd(d["s_mu"], d["s_lv"], d["style_scale"]))]
    return np.array([out0(t, d)] + t)


def out0(t, d):
    return float(F32(d["mse_cof"])) * (t[0] + t[1] + t[2] + t[3]) + float(F32(d["kl_cof"])) * (t[4] + t[5])


def loss_fwd_f32(d, ex, skip_tail=0, swap_scales=False):
    ks, ss = (d["style_scale"], d["kl_scale"]) if swap_scales else (d["kl_scale"], d["style_scale"])
    t = [l1_fwd_f32(d["x%d" % (1 + (k & 1))], d[LOSS_KEYS[2 + k]], d["l1_scale"], skip_tail) for k in range(4)]
    t += [kl_fwd(d["q1_mu"], d["q1_lv"], ks, F32, ex), kl_fwd(d["q2_mu"], d["q2_lv"], ks, F32, ex),
          kl_fwd(d["s_mu"], d["s_lv"], ss, F32, ex)]
    t = [F32(v) for v in t]
    o0 = F32(d["mse_cof"]) * (((t[0] + t[1]) + t[2]) + t[3]) + F32(d["kl_cof"]) * (t[4] + t[5])
    return np.array([o0] + t, F32)


def loss_weights(d, g8, dt=F64):
    """(w[4] of the reconstructions, W1, W2 of the two latent KL terms, Ws of the style KL)."""
    g8, c = np.asarray(g8, dt), {k: dt(F32(d[k])) for k in SCALE_KEYS}
    w = [(g8[0] * c["mse_cof"] + g8[1 + k]) * c["l1_scale"] for k in range(4)]
    return w, (g8[0] * c["kl_cof"] + g8[5]) * c["kl_scale"], (g8[0] * c["kl_cof"] + g8[6]) * c["kl_scale"], g8[7] * c["style_scale"]


def loss_bwd(d, g8, dt=F64, ex=np.exp, tie=0.0):
    """The ten gradients, in the order of dvae_loss_bwd's arguments.  tie: the factor of w at x == recon (0)."""
    w, W1, W2, Ws = loss_weights(d, g8, dt)
    out = []
    for k in range(4):
        x, r = np.asarray(d["x%d" % (1 + (k & 1))], F64), np.asarray(d[LOSS_KEYS[2 + k]], F64)
        out.append(np.where(x > r, -w[k], np.where(x < r, w[k], dt(tie) * w[k])).astype(dt))
    for W, mu, lv in ((W1, "q1_mu", "q1_lv"), (W2, "q2_mu", "q2_lv"), (Ws, "s_mu", "s_lv")):
        m, l = np.asarray(d[mu], dt).reshape(-1), np.asarray(d[lv], dt).reshape(-1)
        out += [W * (dt(-2) * m), W * (dt(1) - ex(l).astype(dt))]
    return out


def colsum(Xm, C, old=None):
    Xm = np.asarray(Xm, F64)
    return Xm[:, :C].sum(0) + (0.0 if old is None else np.asarray(old, F64))


def colsum_ws_f32(Xm, C, old, lose_rows=False):
    """colsum_ws_kernel, addition by addition: row lanes, the lanes' tree, the row blocks per wave, their tree, the output.
    lose_rows: a thread's row count without the + 3 (the last rows of a block are lost)."""
    Xm = np.asarray(Xm, F32)[:, :C]
    R = Xm.shape[0]
    la = colsum_launch(R, C)
    rp, nb = la["rows_pb"], la["nb"]
    pad = np.zeros((nb * rp, C), F32)
    pad[:R] = Xm
    if lose_rows:
        for b in range(nb):
            rows = min(R, (b + 1) * rp) - b * rp
            for rl in range(4):
                keep = max(rows - rl, 0) >> 2
                pad[b * rp + rl + 4 * keep:(b + 1) * rp:4] = 0        # rows of lane rl behind its count
    lanes = pad.reshape(nb, rp // 4, 4, C)
    s = np.zeros((nb, 4, C), F32)
    for i in range(rp // 4):
        s = s + lanes[:, i]
    part = (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])
    ps = np.zeros((4, C), F32)
    for b in range(nb):
        ps[b % 4] = ps[b % 4] + part[b]
    return np.asarray(old, F32) + ((ps[0] + ps[1]) + (ps[2] + ps[3]))


def slab_sum_f32(c, slabs, act, accumulate, skip_window_step=False):
    """v + slab 0 + slab 1 + ... in fp32 in that order, then ReLU (exact) or tanh (float64, NOT rounded: the bound is about
    it).  skip_window_step: slab_add without the `k += 4` behind its window of four (those slabs are added twice)."""
    v = np.asarray(c, F32).copy() if accumulate else np.zeros(np.shape(slabs)[1:], F32)
    ns = len(slabs)
    order = list(range(ns))
    if skip_window_step and (ns % 8) // 4:
        k = 8 * (ns // 8)
        order = list(range(k + 4)) + list(range(k, ns))
    for k in order:
        v = v + np.asarray(slabs[k], F32)
    if act == ACT_RELU:
        return np.where(v > 0, v, F32(0)).astype(F32)
    return np.tanh(v.astype(F64)) if act == ACT_TANH else v


def act_bwd_f32(dz, z, act):
    dz, z = np.asarray(dz, F32), np.asarray(z, F32)
    d = np.where(z > 0, F32(1), F32(0)) if act == ACT_RELU else F32(1) - z * z if act == ACT_TANH else F32(1)
    return (dz * d).astype(F32)


def act_bwd(dz, z, act):
    dz, z = np.asarray(dz, F64), np.asarray(z, F64)
    return dz * ((z > 0).astype(F64) if act == ACT_RELU else 1.0 - z * z if act == ACT_TANH else 1.0)


def conversion_latents(ss, sc, ts, n, m, S, Cn, dt=F64):
    """variational_base_vae.py:281-285: (z_src, z_conv) [n, S + Cn]; ss [n, 2S], sc [n, 2Cn], ts [m, 2S] (mu | logvar)."""
    ss, sc, ts = np.asarray(ss, dt).reshape(n, 2 * S), np.asarray(sc, dt).reshape(n, 2 * Cn), np.asarray(ts, dt).reshape(m, 2 * S)
    a, b = np.zeros(S, dt), np.zeros(S, dt)
    for r in range(n):
        a = a + ss[r, :S]
    for r in range(m):
        b = b + ts[r, :S]
    a, b = a / dt(n), b / dt(m)
    return (np.concatenate([np.tile(a, (n, 1)), sc[:, :Cn]], 1), np.concatenate([np.tile(b, (n, 1)), sc[:, :Cn]], 1))


def mul_div(a, b, c, dt=F64):
    return np.asarray(a, dt) * (np.asarray(b, dt) / np.asarray(c, dt))


# ---- the moves, by index
def mel_to_frames(x1, x2, Bh, C, T):
    x = np.asarray(x1).reshape(Bh, C, T) if x2 is None else np.concatenate([np.asarray(x1).reshape(Bh, C, T), np.asarray(x2).reshape(Bh, C, T)])
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def frames_to_mel(Xf, N, C, T):
    return np.ascontiguousarray(np.asarray(Xf).reshape(T, N, C).transpose(1, 2, 0))


def conv_pack_w(W, Cout, Cin):
    return np.ascontiguousarray(np.asarray(W).reshape(Cout, Cin, 5).transpose(2, 0, 1))


def conv_pack_wt(W, Cout, Cin):
    return np.ascontiguousarray(np.asarray(W).reshape(Cout, Cin, 5).transpose(2, 1, 0))


def conv_unpack_add_w(dWp, dW, Cout, Cin):
    return np.asarray(dW, F32).reshape(Cout, Cin, 5) + np.asarray(dWp, F32).reshape(5, Cout, Cin).transpose(1, 2, 0)


def gather_crop(mels, lens, utt, off, C, T, Lmax):
    """preprocessing/dataset.py:100-109 for a batch: crop [off, off + T) of utterance utt[i], zero behind its length."""
    mels = np.asarray(mels).reshape(-1, C, Lmax)
    out = np.zeros((len(utt), C, T), mels.dtype)
    for i, (u, o) in enumerate(zip(utt, off)):
        k = int(np.clip(lens[u] - o, 0, T))
        out[i, :, :k] = mels[u, :, o:o + k]
    return out


def mel_to_chunks(mel, C, L, T):
    """chunking_mel (variational_base_vae.py:335-348): L // T + 1 chunks of T frames, the last one zero-padded."""
    n = L // T + 1
    pad = np.zeros((C, n * T), np.asarray(mel).dtype)
    pad[:, :L] = np.asarray(mel).reshape(C, -1)[:, :L]
    return np.ascontiguousarray(pad.reshape(C, n, T).transpose(1, 0, 2))


def chunks_to_mel(x, n, C, T, lo, hi, clamp):
    out = np.ascontiguousarray(np.asarray(x).reshape(n, C, T).transpose(1, 0, 2)).reshape(C, n * T)
    return np.clip(out, F32(lo), F32(hi)) if clamp else out


# ------------------------------------------------------------------ the bounds
def tol_z(eps, lv, mu):
    """z = eps exp(0.5 lv) + mu from the fp32 lv, mu the launch stored."""
    return g(X + 2) * np.abs(np.asarray(eps, F64)) * np.exp(0.5 * np.asarray(lv, F64)) + g(1) * np.abs(np.asarray(mu, F64)) + FLOOR


def latent_fwd_bounds(style, content, eps_c, eps_s, Bh, S, Cn):
    """Reference z and its bound; q_mu, q_lv, s_mu, s_lv as the fp32 statement gives them (held bit for bit)."""
    _, q_mu, q_lv, s_mu, s_lv = latent_fwd(style, content, eps_c, eps_s, Bh, S, Cn, F32, exp32(0))
    eps = np.concatenate([np.concatenate([np.asarray(eps_s, F64).reshape(Bh, S)] * 2, 0),
                          _z(eps_c, (2 * Bh, Cn), F64)], 1)
    z = eps * np.exp(0.5 * q_lv.astype(F64)) + q_mu.astype(F64)
    tol = tol_z(eps, q_lv, q_mu)
    if eps_c is None:
        tol[:, S:] = FLOOR                     # a copy of mu
    return {"z": z, "tol_z": tol, "q_mu": q_mu, "q_lv": q_lv, "s_mu": s_mu, "s_lv": s_lv}


def latent_bwd_bounds(style, content, eps_c, eps_s, dz, dq_mu, dq_lv, ds_mu, ds_lv, Bh, S, Cn):
    D = S + Cn
    _, _, q_lv, _, _ = latent_fwd(style, content, None, eps_s, Bh, S, Cn, F32, exp32(0))
    # the logvar the kernel recomputes is the bit-exact fp32 one: the reference runs on it
    st = np.asarray(style, F64).reshape(2 * Bh, 2 * S).copy()
    st[:Bh, S:], st[Bh:, S:] = q_lv[:Bh, :S], q_lv[:Bh, :S]
    ds, dc = latent_bwd(st, content, eps_c, eps_s, dz, dq_mu, dq_lv, ds_mu, ds_lv, Bh, S, Cn)
    a = lambda v, shape: np.abs(_z(v, shape, F64))
    adz, adqm, adql = a(dz, (2 * Bh, D)), a(dq_mu, (2 * Bh, D)), a(dq_lv, (2 * Bh, D))
    es, E = np.abs(np.asarray(eps_s, F64).reshape(Bh, S)), np.exp(0.5 * q_lv.astype(F64))
    ts, tc = np.full_like(ds, FLOOR), np.zeros_like(dc)      # rows >= Bh of dstyle: +0.0
    ts[:Bh, :S] = 0.5 * g(4) * (adz[:Bh, :S] + adz[Bh:, :S] + adqm[:Bh, :S] + adqm[Bh:, :S] + a(ds_mu, (Bh, S))) + FLOOR
    ts[:Bh, S:] = 0.5 * (g(6 + X) * (adz[:Bh, :S] + adz[Bh:, :S]) * es * 0.5 * E[:Bh, :S]
                         + g(3) * (adql[:Bh, :S] + adql[Bh:, :S] + a(ds_lv, (Bh, S)))) + FLOOR
    tc[:, :Cn] = g(1) * (adz[:, S:] + adqm[:, S:]) + FLOOR
    first = 0.0 if eps_c is None else g(3 + X) * adz[:, S:] * a(eps_c, (2 * Bh, Cn)) * 0.5 * E[:, S:]
    tc[:, Cn:] = first + g(1) * adql[:, S:] + FLOOR
    return {"dstyle": ds, "dcontent": dc, "tol_dstyle": ts, "tol_dcontent": tc}


def tol_term(mu, lv):
    mu, lv = np.asarray(mu, F64).reshape(-1), np.asarray(lv, F64).reshape(-1)
    E = np.exp(lv)
    return g(4) * (1.0 + np.abs(lv) + mu * mu + E) + X * EPS32 * (1 + g(4)) * E


def kl_fwd_bounds(mu, lv, scale):
    n = np.asarray(mu).size
    t, a = kl_terms(mu, lv), -(-n // 256) + 26
    out, s = float(kl_fwd(mu, lv, scale)), abs(float(F32(scale)))
    return out, s * (tol_term(mu, lv).sum() + a * EPS64 * np.abs(t).sum()) * (1 + EPS32) + EPS32 * abs(out) + FLOOR


def tol_dlv(A, lv, k):
    """|d(A (1 - exp lv))| with k roundings beside expf's; A: the absolute weight."""
    E = np.exp(np.asarray(lv, F64).reshape(-1))
    return np.abs(A) * (X * EPS32 * (1 + g(k)) * E + g(k) * np.abs(1.0 - E)) + FLOOR


def kl_bwd_bounds(mu, lv, gout, scale):
    dmu, dlv = kl_bwd(mu, lv, float(F32(gout)), float(F32(scale)))
    return {"dmu": dmu, "dlv": dlv, "tol_dmu": g(2) * np.abs(dmu) + FLOOR,
            "tol_dlv": tol_dlv(float(F32(gout)) * float(F32(scale)), lv, 3)}


def l1_fwd_bounds(x, y, scale, final_threads=64):
    n = np.asarray(x).size
    la = l1_launch(n)
    K = 4 * la["trips"] + (1 if la["tail"] else 0)
    a = 9 + -(-la["blocks"] // final_threads) + (6 if final_threads == 64 else 9) + 1 + 16
    out, s = l1_fwd(x, y, scale), abs(float(F32(scale)))
    sabs = np.abs(np.asarray(x, F64) - np.asarray(y, F64)).sum()
    return out, s * (g(K + 1) + a * EPS64) * sabs * (1 + EPS32) + EPS32 * abs(out) + FLOOR


def loss_fwd_bounds(d, dev_out=None):
    """Reference out[8] and the bounds of out[1..7]; with dev_out (the device's own out[8]) out[0] and its bound from the
    device's out[1..6]."""
    ref, tol = np.zeros(8), np.zeros(8)
    for k in range(4):
        ref[1 + k], tol[1 + k] = l1_fwd_bounds(d["x%d" % (1 + (k & 1))], d[LOSS_KEYS[2 + k]], d["l1_scale"], 256)
    for j, (m, l, s) in enumerate((("q1_mu", "q1_lv", "kl_scale"), ("q2_mu", "q2_lv", "kl_scale"), ("s_mu", "s_lv", "style_scale"))):
        ref[5 + j], tol[5 + j] = kl_fwd_bounds(d[m], d[l], d[s])
    t = ref[1:] if dev_out is None else np.asarray(dev_out, F64)[1:]
    ref[0] = out0(list(t), d)
    tol[0] = g(5) * (abs(float(F32(d["mse_cof"]))) * np.abs(t[:4]).sum() + abs(float(F32(d["kl_cof"]))) * (abs(t[4]) + abs(t[5]))) + FLOOR
    return ref, tol


def loss_bwd_bounds(d, g8):
    """Reference gradients (order of dvae_loss_bwd) and bounds; for the four reconstructions the bound is that of the one
    weight (a scalar), the pattern -sign(x - recon) w is exact."""
    g8 = np.asarray(g8, F32)
    ref = loss_bwd(d, g8.astype(F64))
    c = {k: abs(float(F32(d[k]))) for k in SCALE_KEYS}
    a8 = np.abs(g8.astype(F64))
    aw = [(a8[0] * c["mse_cof"] + a8[1 + k]) * c["l1_scale"] for k in range(4)]
    A = [(a8[0] * c["kl_cof"] + a8[5]) * c["kl_scale"], (a8[0] * c["kl_cof"] + a8[6]) * c["kl_scale"], a8[7] * c["style_scale"]]
    tol = [g(3) * aw[k] + FLOOR for k in range(4)]
    for j, (m, l) in enumerate((("q1_mu", "q1_lv"), ("q2_mu", "q2_lv"), ("s_mu", "s_lv"))):
        tol += [g(4) * A[j] * np.abs(2.0 * np.asarray(d[m], F64).reshape(-1)) + FLOOR, tol_dlv(A[j], d[l], 4)]
    return ref, tol


def colsum_bounds(Xm, C, old, variant="ws"):
    """variant: ws, atomic, deterministic."""
    Xm = np.asarray(Xm, F64)[:, :C]
    R = Xm.shape[0]
    la = colsum_launch(R, C, variant == "deterministic")
    rows = min(R, la["rows_pb"])
    K = -(-rows // 4) + (-(-la["nb"] // 4) + 5 if variant == "ws" else 2 + la["nb"])
    old = np.zeros(C) if old is None else np.asarray(old, F64)
    return Xm.sum(0) + old, g(K) * (np.abs(Xm).sum(0) + np.abs(old)) + FLOOR


def tol_tanh(u):
    return TANHF_ROUNDINGS * EPS32 * np.abs(np.tanh(np.asarray(u, F64))) + FLOOR


def tol_act_bwd_tanh(dz, z):
    dz, zz = np.asarray(dz, F64), np.asarray(z, F64) ** 2
    return EPS32 * np.abs(dz) * (zz + np.abs(1.0 - zz)) + EPS32 * np.abs(dz * (1.0 - zz)) + FLOOR


def conversion_bounds(ss, sc, ts, n, m, S, Cn):
    zs, zc = conversion_latents(ss, sc, ts, n, m, S, Cn)
    ss, ts = np.abs(np.asarray(ss, F64).reshape(n, 2 * S)[:, :S]), np.abs(np.asarray(ts, F64).reshape(m, 2 * S)[:, :S])
    return zs, zc, g(n - 1 + DIV_ROUNDINGS) * ss.sum(0) / n + FLOOR, g(m - 1 + DIV_ROUNDINGS) * ts.sum(0) / m + FLOOR


def mul_div_bounds(a, b, c):
    r = mul_div(a, b, c)
    return r, g(DIV_ROUNDINGS + 1) * np.abs(r) + FLOOR


# ------------------------------------------------------------------ inputs of the tests (CPU and GPU alike)
def _f32(a):
    return np.ascontiguousarray(a, dtype=F32)


def edge_lv(rs, n, wide=True):
    """Log-variances: uniform over [-30, 30] (wide; every fifth one and all of the narrow form in [-2, 2], where exp(lv) is of
    the order of the other terms: a sum over the wide form is bounded by its largest exp alone) with the edges mixed in at
    the front: 0, -0.0, +-2^-24 and +-2^-25 (half-ulp neighbours of the 1 they are added to), the smallest denormals, +-30."""
    v = rs.uniform(-30, 30, n) if wide else rs.uniform(-2, 2, n)
    v[1::5] = rs.uniform(-2, 2, len(v[1::5]))
    e = [0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 2.0 ** -149, -2.0 ** -149] + ([30.0, -30.0] if wide else [])
    k = min(n, len(e))
    v[:k] = e[:k]
    return _f32(v)


def edge_mu(rs, n):
    v = rs.uniform(-3, 3, n)
    e = [0.0, 0.0, -0.0, 2.0 ** -24, 1.0, 0.0, 2.0 ** -75, -2.0 ** -149, 0.0, 0.0]
    k = min(n, len(e))
    v[:k] = e[:k]
    return _f32(v)


def edge_pair(rs, n, width=1.0):
    """(x, r) for the L1 kernels: full significands, and from index 0 on (as far as n - 1 reaches): a tie, one ulp up, one ulp
    down, a denormal difference, -0.0 against +0.0, a tie at a negative value, +0.0 against the smallest denormal; ties at
    every seventh element from 10 on, a one-ulp difference at n - 2.  The last element keeps a full difference: a lost tail
    shows in the sum."""
    x, r = _f32(rs.uniform(0, 1, n)), _f32(rs.uniform(-width, width, n))
    last, one = (x[n - 1], r[n - 1]), F32(1)
    ex = [(x[0], x[0]), (F32(0.75), np.nextafter(F32(0.75), one)), (F32(0.75), np.nextafter(F32(0.75), -one)),
          (F32(2.0 ** -125), np.nextafter(F32(2.0 ** -125), one)), (F32(-0.0), F32(0.0)), (F32(-0.375), F32(-0.375)),
          (F32(0.0), F32(2.0 ** -149))]
    for i, (a, b) in enumerate(ex[:n]):
        x[i], r[i] = a, b
    x[10::7] = r[10::7]
    if n > len(ex) + 1:
        x[n - 2] = np.nextafter(r[n - 2], one)
    x[n - 1], r[n - 1] = last
    return x, r


def int_pair(rs, n):
    """Class E of the L1 kernels: integers in [-4, 4]: every fp32 sum below is exact (n <= 2^21), ties included."""
    return _f32(rs.randint(-4, 5, n)), _f32(rs.randint(-4, 5, n))


def colsum_inputs(R, C, ld, bf16, cls, seed):
    """X [R, ld] with NaN in the columns C..ld.  Class R: full significands (bf16-representable for bf16) in +-[0, 2].
    Class E: integers in [-3, 3] times 2^(row block % 4), row blocks of 512 rows: every sum is exact (24 R < 2^24) and a lost
    or doubled row or row block changes the integer."""
    rs = np.random.RandomState(seed)
    if cls == "E":
        v = rs.randint(-3, 4, (R, C)) * (2.0 ** ((np.arange(R) // 512) % 4))[:, None]
    else:
        v = rs.uniform(-2, 2, (R, C))
    v = _f32(v)
    if bf16:
        v = (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)
    Xm = np.full((R, ld), np.nan, F32)
    Xm[:, :C] = v
    return Xm


def slab_inputs(n, nslab, stride, cls, seed):
    """(c [n], slab storage [max(nslab, 1) * stride] with NaN between the slabs, list of the nslab slab views [n]).  Class E:
    slab k holds 2^(k % 20) times integers in [-3, 3] and c integers: every partial sum is exact."""
    rs = np.random.RandomState(seed)
    store = np.full(max(nslab, 1) * stride, np.nan, F32)
    for k in range(nslab):
        store[k * stride:k * stride + n] = rs.randint(-3, 4, n) * 2.0 ** (k % 20) if cls == "E" else rs.uniform(-1, 1, n)
    c = _f32(rs.randint(-3, 4, n)) if cls == "E" else _f32(rs.uniform(-1, 1, n))
    if cls == "R" and n >= 8:
        c[:4] = [0.0, -0.0, 2.0 ** -149, -1.0]
        if nslab:
            store[:4] = [-0.0, -0.0, -2.0 ** -149, 1.0]          # sums of exactly -0.0, 0, 0 in the first elements
            for k in range(1, nslab):
                store[k * stride:k * stride + 4] = [-0.0, 0.0, 0.0, 0.0]
    return c, store, [store[k * stride:k * stride + n] for k in range(nslab)]


def latent_inputs(Bh, S, Cn, seed):
    rs = np.random.RandomState(seed)
    D = S + Cn
    style, content = np.zeros((2 * Bh, 2 * S), F32), np.zeros((2 * Bh, 2 * Cn), F32)
    style[:, :S], style[:, S:] = edge_mu(rs, 2 * Bh * S).reshape(2 * Bh, S), edge_lv(rs, 2 * Bh * S).reshape(2 * Bh, S)
    content[:, :Cn], content[:, Cn:] = edge_mu(rs, 2 * Bh * Cn).reshape(2 * Bh, Cn), edge_lv(rs, 2 * Bh * Cn).reshape(2 * Bh, Cn)
    u = lambda *s: _f32(rs.uniform(-1, 1, s))
    return {"style": style, "content": content, "eps_c": _f32(rs.standard_normal((2 * Bh, Cn))), "eps_s": _f32(rs.standard_normal((Bh, S))),
            "dz": u(2 * Bh, D), "dq_mu": u(2 * Bh, D), "dq_lv": u(2 * Bh, D), "ds_mu": u(Bh, S), "ds_lv": u(Bh, S)}


def loss_inputs(n, nq, ns, cls, seed, wide=True):
    """The arrays and scalars of dvae_loss_desc_t.  Class E: integer x / recon, logvar 0 is not assumed exact: only the four
    L1 entries are compared bit for bit there."""
    rs = np.random.RandomState(seed)
    d = {}
    if cls == "E":
        for k, key in enumerate(LOSS_KEYS[:6]):
            d[key] = _f32(rs.randint(-4, 5, n))
    else:
        x1, r1 = edge_pair(rs, n)
        x2, r2 = edge_pair(rs, n, 0.5)
        d.update(x1=x1, x2=x2, recon1=r1, recon2=r2, recon1_hat=_f32(r1 + rs.uniform(-0.1, 0.1, n)),
                 recon2_hat=_f32(rs.uniform(-1, 1, n)))
        d["recon1_hat"][::3], d["recon2_hat"][1::3] = x1[::3], x2[1::3]
        d["recon1_hat"][n - 1], d["recon2_hat"][n - 1] = x1[n - 1] + F32(0.25), x2[n - 1] - F32(0.25)
    for m, l, k in (("q1_mu", "q1_lv", nq), ("q2_mu", "q2_lv", nq), ("s_mu", "s_lv", ns)):
        d[m], d[l] = edge_mu(rs, k), edge_lv(rs, k, wide)
    d.update(n=n, nq=nq, ns=ns, l1_scale=F32(1.0 / 64 if cls == "E" else 1.0 / 7), kl_scale=F32(-0.5 / 5),
             style_scale=F32(-1.0 / 7), mse_cof=F32(10.0), kl_cof=F32(3.0))
    return d


G8 = {"ones": _f32(np.ones(8)), "random": _f32(np.random.RandomState(8).uniform(-2, 2, 8)), "total": _f32([1, 0, 0, 0, 0, 0, 0, 0])}

# name -> shape, and what tests/test_elem_ref.py asserts the shape reaches (by the launch arithmetic above)
CASES = {
    "latent": {"one": (1, 1, 1), "model": (5, MODEL_S, MODEL_CN), "two_blocks": (43, 1, 2)},
    "kl": [1, 255, 256, 257, 4099],
    # 4099: five workgroups, the last one idle; 524288: every thread exactly one trip, no tail; 524291: the same + a tail of 3; 524292: the first second trip;
    # 1048583: three forward trips, the second backward trip, a tail of 3
    "l1": [1, 3, 4, 5, 1023, 4099, 524288, 524291, 524292, 1048583],
    "loss_nq_ns": [(1, 1), (255, 300), (257, 1)],
    "colsum_C": [1, 3, 80, 255, 258, 520],
    "colsum_R": [1, 3, 511, 512, 513, 1025, 8192],
    "colsum_1024": (524288, 8),
    "colsum_xcd": (8192, 512),
    "slab_nslab": [0, 1, 3, 4, 7, 8, 9, 12, 13, 17],
    "fold_entries": 70,
    "act": [1, 257, 524293],
    "frames": [(1, 1, 1), (2, 33, 65), (3, 80, 31), (3, 80, 32), (3, 80, 33)],
    "permute": [(3, 5, 4), (1, 7, 8), (6, 1, 132)],
    "transpose": [(1, 1), (31, 33), (100, 260), (1, 1000)],
    "conv_pack": [(1, 1), (33, 31), (80, 512), (512, 80)],
    "conversion": [(1, 1), (7, 3)],
    "mul_div": [1, 1000],
}


def fold_table(seed=70):
    """70 entries (two launches of slab_fold): n a multiple of 4 from 4 up, nslab 1 ... 17, stride == n or n + 8."""
    rs = np.random.RandomState(seed)
    tab = []
    for e in range(CASES["fold_entries"]):
        n = 4 * (1 + (e * 37) % 300) if e else 4
        tab.append((n, 1 + e % 17, n + (8 if e % 3 == 0 else 0), int(rs.randint(1 << 30))))
    return tab
