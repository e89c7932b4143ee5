"""Float64 numpy restatement of the i-vector speaker embeddings (dvae_amd.ivector): the
per-utterance statistics from a given gamma, the Gram matrices, the posterior by an explicit Cholesky walk, the accumulators,
the M-step, minimum divergence, the backend and the equal error rate, and the error bounds the kernels are held to.  The
bounds come from operation counts and eps64 = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm
10.4 with eq. 10.7), not from what a kernel gives.  Not a test module: tests/test_ivector_ref.py and
tests/test_hip_ivector.py use it.  Shapes: n [U, K], f [U, K D], T [K D, R] (row c D + d), P [K, R, R], w [U, R],
S [U, R, R], ll [U].
"""
import numpy as np

from ref_common import EPS64, F, F64, FLOOR  # noqa: F401

N_FLOOR = 1e-3          # a component with sum_u n_uc below it keeps its rows of T
INIT_SCALE = 0.1        # the initial T is standard normal times this
EIG_FLOOR = 1e-10       # the backend's eigenvalues are floored at this times the largest


# ---------------------------------------------------------------------------------------------------------- statistics
def utt_sums(x, gamma, segs):
    """n [U, K], g [U, K, D] and the same sums over |term| (an, ag), float64, from gamma [N, K] and x [N, D]"""
    x, gamma = np.asarray(x, F64), np.asarray(gamma, F64)
    U, K, D = len(segs), gamma.shape[1], x.shape[1]
    n, g, an, ag = np.zeros((U, K)), np.zeros((U, K, D)), np.zeros((U, K)), np.zeros((U, K, D))
    for u, (r0, c) in enumerate(segs):
        gm, xs = gamma[r0:r0 + c], x[r0:r0 + c]
        n[u], g[u] = gm.sum(axis=0), gm.T @ xs
        an[u], ag[u] = np.abs(gm).sum(axis=0), np.abs(gm).T @ np.abs(xs)
    return n, g, an, ag


def centre_whiten(n, g, mu, prec):
    """f [U, K D] = (g - n mu) sqrt(prec), mu and prec the fp32 tables widened exactly.  The square root is float64's
    (correctly rounded, as the kernel's); the product, the difference and the product are carried in long double and
    rounded once at the end, so that the kernel's three roundings are the only ones between the two."""
    LD = np.longdouble
    mu, sq = np.asarray(mu, F64).astype(LD), np.sqrt(np.asarray(prec, F64)).astype(LD)
    n, g = np.asarray(n, F64).astype(LD), np.asarray(g, F64).astype(LD)
    return ((g - n[:, :, None] * mu[None]) * sq[None]).astype(F64).reshape(len(n), -1)


def sum_bound(n_terms, abs_sum):
    """|float64 sum in any order - exact| <= (n + 2) 2^-53 sum |term| (the products are one rounding each)"""
    return (np.asarray(n_terms, F64) + 2) * EPS64 * np.asarray(abs_sum, F64)


def stats_bounds(counts, an, ag, mu, prec):
    """-> (bound on n [U, K], bound on f [U, K D]) against the exact sums of the same gamma: the summation bound, carried
    through f = (g - n mu) s, plus the three roundings of centring and whitening (product, difference, product; the
    square root is correctly rounded on both sides), each relative to at most s (|g| + |n mu|), plus the one rounding of
    the reference's own result to float64"""
    cnt = np.asarray(counts, F64).reshape(-1, 1)
    mu, sq = np.abs(np.asarray(mu, F64)), np.sqrt(np.asarray(prec, F64))
    bn, bg = sum_bound(cnt, an), sum_bound(cnt[:, :, None], ag)
    mag = ag + an[:, :, None] * mu[None]
    bf = sq[None] * (bg + bn[:, :, None] * mu[None]) + (3.0 + 1.0) * EPS64 * (1.0 + 8 * EPS64) * sq[None] * (mag + bg + bn[:, :, None] * mu[None])
    return bn + FLOOR, bf.reshape(len(bn), -1) + FLOOR


# ----------------------------------------------------------------------------------------------------------- posterior
def gram(T, K, D):
    """P [K, R, R], P_c = T_c^T T_c"""
    T = np.asarray(T, F64)
    Tc = T.reshape(K, D, T.shape[1])
    return np.einsum("cdi,cdj->cij", Tc, Tc)


def form(n, f, T, P):
    """L [U, R, R] = I + sum_c n_uc P_c, b [U, R] = T^T f_u"""
    n, f, T, P = (np.asarray(v, F64) for v in (n, f, T, P))
    return np.eye(T.shape[1])[None] + np.einsum("uc,cij->uij", n, P), f @ T


def cholesky_walk(L):
    """the lower factor G of one L by columns, the inner products k ascending (the kernel's walk)"""
    R = L.shape[0]
    G = np.zeros((R, R))
    for j in range(R):
        s = L[j:, j].copy()
        for k in range(j):
            s = s - G[j:, k] * G[j, k]
        with np.errstate(invalid="ignore"):
            G[j, j] = np.sqrt(s[0])
        G[j + 1:, j] = s[1:] / G[j, j]
    return G


def solve_walk(G, rhs):
    """G G^T x = rhs by the two substitutions, rows ascending then descending; rhs [R] or [R, m]"""
    R = G.shape[0]
    x = np.array(rhs, F64)
    for i in range(R):
        for k in range(i):
            x[i] = x[i] - G[i, k] * x[k]
        x[i] = x[i] / G[i, i]
    for i in range(R - 1, -1, -1):
        for k in range(i + 1, R):
            x[i] = x[i] - G[k, i] * x[k]
        x[i] = x[i] / G[i, i]
    return x


def posterior(n, f, T, P):
    """the explicit walk -> dict(w, S, ll, L, b, inv)"""
    L, b = form(n, f, T, P)
    U, R = b.shape
    w, inv, ll = np.zeros((U, R)), np.zeros((U, R, R)), np.zeros(U)
    for u in range(U):
        G = cholesky_walk(L[u])
        w[u] = solve_walk(G, b[u])
        inv[u] = solve_walk(G, np.eye(R))
        with np.errstate(invalid="ignore", divide="ignore"):
            ll[u] = 0.5 * (b[u] @ w[u]) - np.log(np.diag(G)).sum()
    return dict(w=w, S=inv + w[:, :, None] * w[:, None, :], ll=ll, L=L, b=b, inv=inv)


def posterior_linalg(n, f, T, P):
    """the same by numpy.linalg (LAPACK: other orders) -> dict(w, S, ll, L, b, inv)"""
    L, b = form(n, f, T, P)
    w = np.linalg.solve(L, b[:, :, None])[:, :, 0]
    inv = np.linalg.inv(L)
    ll = 0.5 * np.einsum("ur,ur->u", b, w) - 0.5 * np.linalg.slogdet(L)[1]
    return dict(w=w, S=inv + w[:, :, None] * w[:, None, :], ll=ll, L=L, b=b, inv=inv)


def eps_b(K, D, R):
    """[(3 R + 1) R + (K + 2) + K D] 2^-53: gamma_{3R+1} of the Cholesky solve (Thm 10.4) times the R of eq. 10.7
    (|| |G| |G^T| ||_2 <= R ||L||_2), plus forming L (K terms and the identity) and b (K D terms)"""
    return ((3 * R + 1) * R + (K + 2) + K * D) * EPS64


def norm2(M):
    return float(np.linalg.norm(M, 2))


def backward_ratios(L64, b64, w, S, K, D, R):
    """for one utterance: (||b - L w|| / (eps_b ||L|| ||w||), the worst column of ||e_c - L (S - w w^T)_c|| over its bound).
    The inverse is recovered from S in float64: the kernel's rounding of S = X + w w^T (one fma) and the product and
    difference here add 3 eps (|S_ij| + |w_i w_j|) per element to the column's bound."""
    e, nl = eps_b(K, D, R), norm2(L64)
    rw = np.linalg.norm(b64 - L64 @ w) / max(e * nl * np.linalg.norm(w), FLOOR)
    if S is None:
        return rw, 0.0
    ww = np.outer(w, w)
    X = S - ww
    res = np.linalg.norm(np.eye(R) - L64 @ X, axis=0)
    tol = nl * (e * np.linalg.norm(X, axis=0) + 3.0 * EPS64 * (np.linalg.norm(S, axis=0) + np.linalg.norm(ww, axis=0)))
    return rw, float((res / np.maximum(tol, FLOOR)).max())


def forward_bounds(L64, w64, ll64, K, D, R):
    """for one utterance: (bound on ||w - w64||_2, bound on |ll - ll64|, kappa_2(L64))"""
    kappa = float(np.linalg.cond(L64, 2))
    e = eps_b(K, D, R)
    return 2.0 * kappa * e * np.linalg.norm(w64) + FLOOR, R * kappa * e * (1.0 + abs(ll64)), kappa


def s_forward_bound(L64, w64, inv64, K, D, R):
    """bound on ||S - S64||_F: the inverse's columns by the forward form, w w^T by the product rule, one rounding of S"""
    bw, _, kappa = forward_bounds(L64, w64, 0.0, K, D, R)
    nw = np.linalg.norm(w64)
    return (2.0 * kappa * eps_b(K, D, R) * np.linalg.norm(inv64) + 2.0 * nw * bw + bw * bw +
            EPS64 * (np.linalg.norm(inv64) + nw * nw) + FLOOR)


# --------------------------------------------------------------------------------------------------------------- EM
def accumulators(n, f, w, S):
    """A [K, R, R] = sum_u n_uc S_u, C [K D, R] = sum_u f_u w_u^T, Ssum [R, R]"""
    n, f, w, S = (np.asarray(v, F64) for v in (n, f, w, S))
    return np.einsum("uc,uij->cij", n, S), f.T @ w, S.sum(axis=0)


def accumulators_abs(n, f, w, S):
    return accumulators(np.abs(n), np.abs(f), np.abs(w), np.abs(S))


def m_step(T, A, C, nsum, K, D, n_floor=N_FLOOR):
    """T_c = C_c A_c^-1 (T_c A_c = C_c by numpy.linalg.solve); a component with nsum_c < n_floor keeps its rows"""
    T = np.array(T, F64)
    for c in range(K):
        if nsum[c] >= n_floor:
            T[c * D:(c + 1) * D] = np.linalg.solve(A[c].T, C[c * D:(c + 1) * D].T).T
    return T


def min_divergence(T, Ssum, U):
    """T chol(Ssum / U): the factor's second moment becomes the identity, the likelihood does not fall"""
    return T @ np.linalg.cholesky(Ssum / U)


def init_T(K, D, R, seed, scale=INIT_SCALE):
    return np.random.default_rng(seed).standard_normal((K * D, R)) * scale


def em_step(n, f, T, K, D, min_div=True, n_floor=N_FLOOR, post=posterior):
    """one iteration from T -> (next T, sum_u ll_u under T, the posterior)"""
    p = post(n, f, T, gram(T, K, D))
    A, C, Ssum = accumulators(n, f, p["w"], p["S"])
    T2 = m_step(T, A, C, np.asarray(n, F64).sum(axis=0), K, D, n_floor)
    if min_div:
        T2 = min_divergence(T2, Ssum, len(n))
    return T2, float(p["ll"].sum()), p


def em(n, f, K, D, R, iters, seed=0, min_div=True, n_floor=N_FLOOR, scale=INIT_SCALE, post=posterior_linalg):
    """-> (T, [sum_u ll_u / U per iteration])"""
    T, lls = init_T(K, D, R, seed, scale), []
    for _ in range(iters):
        T, ll, _ = em_step(n, f, T, K, D, min_div, n_floor, post)
        lls.append(ll / len(n))
    return T, lls


def em_step_bound(n, f, T, K, D, min_div=True):
    """bound [K D, R] (one number per component, broadcast) on |T' - T'64| of one iteration from the SAME T, n, f, when w and
    S carry the forward bounds and the accumulators the summation bound; first order, doubled for the higher orders, plus
    1e-13 (1 + |T'|) for the host's own solves (which run on slightly different A and C)."""
    n, f = np.asarray(n, F64), np.asarray(f, F64)
    U, R = len(n), T.shape[1]
    p = posterior_linalg(n, f, T, gram(T, K, D))
    dw, dS = np.zeros(U), np.zeros(U)
    for u in range(U):
        dw[u] = forward_bounds(p["L"][u], p["w"][u], 0.0, K, D, R)[0]
        dS[u] = s_forward_bound(p["L"][u], p["w"][u], p["inv"][u], K, D, R)
    A, C, Ssum = accumulators(n, f, p["w"], p["S"])
    aA, aC, aS = accumulators_abs(n, f, p["w"], p["S"])
    sb = (U + 2) * EPS64
    dA = np.array([np.sum(np.abs(n[:, c]) * dS) + sb * np.linalg.norm(aA[c]) for c in range(K)])
    dC = np.array([np.sum(np.linalg.norm(f[:, c * D:(c + 1) * D], axis=1) * dw) + sb * np.linalg.norm(aC[c * D:(c + 1) * D])
                   for c in range(K)])
    dSs = dS.sum() + sb * np.linalg.norm(aS)
    T2 = m_step(T, A, C, n.sum(axis=0), K, D)
    out = np.zeros_like(T2)
    for c in range(K):
        Tc = T2[c * D:(c + 1) * D]
        ainv = norm2(np.linalg.inv(A[c]))
        out[c * D:(c + 1) * D] = 2.0 * ainv * (dC[c] + np.linalg.norm(Tc) * dA[c])
    if min_div:
        M = Ssum / U
        J = np.linalg.cholesky(M)
        dJ = 2.0 * np.linalg.cond(M) * (dSs / U) / norm2(M) * np.linalg.norm(J)      # Sun (1991): first order, doubled
        out = out * norm2(J) + np.linalg.norm(T2, axis=1, keepdims=True) * dJ
        T2 = T2 @ J
    return out + 1e-13 * (1.0 + np.abs(T2))


# ---------------------------------------------------------------------------------------------------------- backend
def backend_fit(w, eig_floor=EIG_FLOOR):
    """-> (mean [R], W [R, R]): y = (w - mean) W whitens the training i-vectors' total covariance"""
    w = np.asarray(w, F64)
    mean = w.mean(axis=0)
    c = w - mean
    lam, V = np.linalg.eigh(c.T @ c / len(w))
    lam = np.maximum(lam, eig_floor * lam.max())
    return mean, V / np.sqrt(lam)[None]


def backend_transform(w, mean, W):
    y = (np.asarray(w, F64) - mean) @ W
    return y / np.maximum(np.linalg.norm(y, axis=-1, keepdims=True), FLOOR)


def speaker_model(ys):
    m = np.asarray(ys, F64).mean(axis=0)
    return m / max(np.linalg.norm(m), FLOOR)


def cosine(utts, speakers):
    a, b = np.asarray(utts, F64), np.asarray(speakers, F64)
    return (a @ b.T) / np.maximum(np.linalg.norm(a, axis=1)[:, None] * np.linalg.norm(b, axis=1)[None], FLOOR)


# --------------------------------------------------------------------------------------------------------------- EER
def cross(far, frr, thr):
    """operating points in threshold order (far falls, frr rises) -> (eer, threshold) where they cross, interpolated
    linearly between the two adjacent points"""
    d = np.asarray(frr, F64) - np.asarray(far, F64)
    i = int(np.nonzero(d >= 0)[0][0])
    if i == 0 or d[i] == 0:
        return float(frr[i]), float(thr[i])
    s = -d[i - 1] / (d[i] - d[i - 1])
    return float(frr[i - 1] + s * (frr[i] - frr[i - 1])), float(thr[i - 1] + s * (thr[i] - thr[i - 1]))


def eer(target, nontarget):
    """by the sorted scores.  Operating point k accepts score >= t_k, t_k the distinct scores ascending; the last one
    accepts nothing (its threshold is the largest score again)."""
    tar, non = np.sort(np.asarray(target, F64)), np.sort(np.asarray(nontarget, F64))
    if tar.size == 0 or non.size == 0 or np.isnan(tar).any() or np.isnan(non).any():
        raise ValueError("eer: needs target and non-target scores without NaN")
    thr = np.unique(np.concatenate([tar, non]))
    frr = np.concatenate([np.searchsorted(tar, thr, side="left"), [tar.size]]) / tar.size
    far = np.concatenate([non.size - np.searchsorted(non, thr, side="left"), [0]]) / non.size
    return cross(far, frr, np.concatenate([thr, thr[-1:]]))


def eer_brute(target, nontarget):
    """the same by a sweep over every distinct score as the threshold, counted one score at a time"""
    tar, non = [float(v) for v in target], [float(v) for v in nontarget]
    thr = sorted(set(tar + non))
    far = [sum(1 for v in non if v >= t) / len(non) for t in thr] + [0.0]
    frr = [sum(1 for v in tar if v < t) / len(tar) for t in thr] + [1.0]
    return cross(np.array(far), np.array(frr), np.array(thr + thr[-1:]))


# ----------------------------------------------------------------------------------------------- the planted speakers
def planted(seed=0, K=4, D=3, R=2, speakers=6, utts=8, frames=60):
    """A UBM of K well separated components and `speakers` speakers whose component means are shifted by T0 w_speaker (in
    the whitened space: by sigma_cd (T0 w)_cd).  -> dict(ubm (w, mu, var), T0, W [speakers, R], x [N, D] fp32-representable,
    segs [U, 2], speaker [U]); utterances speaker-major."""
    rs = np.random.RandomState(seed)
    mu = rs.randn(K, D) * 6.0
    var = rs.uniform(0.5, 1.5, (K, D))
    wts = np.full(K, 1.0 / K)
    T0 = rs.randn(K * D, R) * 0.8
    ang = 2.0 * np.pi * np.arange(speakers) / speakers      # evenly spread directions: a cosine tells them apart
    W = np.zeros((speakers, R))
    W[:, 0], W[:, 1 % R] = 2.0 * np.cos(ang), 2.0 * np.sin(ang)
    xs, segs, spk = [], [], []
    for s in range(speakers):
        shift = (T0 @ W[s]).reshape(K, D) * np.sqrt(var)
        for _ in range(utts):
            comp = rs.randint(0, K, frames)
            xs.append(mu[comp] + shift[comp] + rs.randn(frames, D) * np.sqrt(var[comp]))
            segs.append((len(segs) * frames, frames))
            spk.append(s)
    x = np.concatenate(xs).astype(F).astype(F64)
    return dict(ubm=(wts, mu, var), T0=T0, W=W, x=x, segs=np.array(segs, np.int64), speaker=np.array(spk), K=K, D=D, R=R,
                utts=utts)


def identify(w_train, spk_train, w_test):
    """backend on the training i-vectors, one model per speaker from them -> (cosine [n_test, n_speakers], mean, W)"""
    mean, W = backend_fit(w_train)
    y = backend_transform(w_train, mean, W)
    models = np.stack([speaker_model(y[spk_train == s]) for s in np.unique(spk_train)])
    return cosine(backend_transform(w_test, mean, W), models), mean, W


def margin(cos, spk):
    """the smallest (own speaker's cosine - the best other's)"""
    cos = np.asarray(cos, F64)
    own = cos[np.arange(len(spk)), spk]
    other = np.where(np.arange(cos.shape[1])[None] == np.asarray(spk)[:, None], -np.inf, cos).max(axis=1)
    return float((own - other).min())


def cosine_bound(dw, w, mean, W):
    """bound on the change of any cosine when every i-vector (training, enrolment and test alike) moves by at most dw in
    norm: y = (w - mean) W moves by at most 2 ||W|| dw (the mean moves too; W's own change is second to that for a
    well-conditioned covariance and is covered by the factor 100 the tests demand of the margin), length normalisation
    divides by ||y||, and a cosine of unit vectors moves by at most the sum of both vectors' changes."""
    y = (np.asarray(w, F64) - mean) @ W
    return float(2.0 * (2.0 * norm2(W) * dw / np.linalg.norm(y, axis=1).min()))


def w_input_bound(dn, df, T, P, L, w):
    """bound on the change of one utterance's w = L^-1 b when n moves by at most dn [K] and f by at most df [K D]
    (elementwise): |dw| <= ||L^-1||_2 (|| |T|^T df || + sum_c dn_c ||P_c||_2 ||w||); first order, doubled"""
    T, P = np.asarray(T, F64), np.asarray(P, F64)
    linv = 1.0 / float(np.linalg.eigvalsh(L)[0])
    return 2.0 * linv * (np.linalg.norm(np.abs(T).T @ df) + sum(dn[c] * norm2(P[c]) for c in range(len(dn))) * np.linalg.norm(w))


def gamma_input_bounds(gb, x, mu, prec):
    """a segment's gamma moves by at most gb [count, K] elementwise -> (dn [K], df [K D]): f = sum_t gamma_t (x_t - mu) s in
    exact arithmetic, so its change is at most sum_t gb_t |x_t - mu| s"""
    x, mu, sq = np.asarray(x, F64), np.asarray(mu, F64), np.sqrt(np.asarray(prec, F64))
    return gb.sum(axis=0), (np.einsum("tk,tkd->kd", gb, np.abs(x[:, None, :] - mu[None])) * sq).reshape(-1)


# ------------------------------------------------------------------------------------- inputs of the posterior's suites
POSTERIOR_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 2), (7, 4, 5, 3), (9, 5, 7, 17), (33, 64, 23, 32), (5, 8, 3, 33), (3, 256, 32, 64)]
N_SCALE = 1e6


def posterior_inputs(U, K, D, R, seed=0):
    """n [U, K] >= 0 (an utterance of about 200 frames spread over the components), f [U, K D] of the size the whitened
    first-order statistics of that many frames have, T [K D, R] whose last column is zero (R >= 2).  The last utterance is
    all zero (U >= 2); utterance 1 has its n multiplied by 1e6 (U >= 3): with T's zero column, L then has eigenvalues from 1
    to about 1e6 ||sum_c n_c P_c||."""
    rs = np.random.RandomState(1000 * R + 10 * K + U + seed)
    n = rs.dirichlet(np.ones(K), U) * 200.0
    f = rs.randn(U, K * D) * np.sqrt(np.repeat(n, D, axis=1))
    T = rs.randn(K * D, R) * 0.3
    if R >= 2:
        T[:, -1] = 0.0
    if U >= 3:
        n[1] *= N_SCALE
    if U >= 2:
        n[-1], f[-1] = 0.0, 0.0
    return n, f, T
