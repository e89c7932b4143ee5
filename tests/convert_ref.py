"""The float64 restatement of whole-utterance conversion (dvae_amd/convert.py, the three window kernels of csrc/elem.hip,
DESIGN.md section 4.12) and the bounds a launch is held to.  Not a test module: tests/test_convert_ref.py checks the
restatement and the host plan on the CPU, tests/test_hip_convert.py holds the kernels and the engine to it.  numpy only; the
statements are the issue's, the bounds are derived here; neither follows what some code computes.

Plan.  An utterance of L frames, windows of T, 1 <= hop <= T: starts = range(0, L - T, hop) + [max(0, L - T)].  A packed batch:
utterance u owns columns [col0, col0 + L) of [C, ld], col0 a multiple of 4; utt[u] = {col0, L, win0, nwin}, win[w] = {utt,
frame0}, padding windows {-1, 0} fill the list to a multiple of the forward batch: window i is row i % batch of forward
i // batch.

mel_to_windows: a copy (zeros beyond L and in padding windows): bits.
window_latents: m_g = sums[g][:S] / counts[g]; z = fp32((1 - mix) m_src + mix m_trg).  All float64 until the store.  At mix = 0
    and mix = 1 one product is the other mean times exactly 1, the other is an exact zero, and a fused multiply-add changes
    nothing: the bits of fp32(m).  In between the two quotients round once each in float64, the products once, the sum once — or
    the last product not at all if the compiler fuses it: 4 eps64 of the absolute terms cover either — and the store rounds once
    to fp32:   |z' - z| <= eps32 |z| + 4 eps64 (|(1 - mix) m_src| + |mix m_trg|) + FLOOR,   under one fp32 ulp.
overlap_add, frame t covered by windows k = 1..n (n >= 2) in window order: num = sum_k w[j_k] y_k, den = sum_k w[j_k], j_k = t -
    frame0_k, with w the fp32 table as uploaded (taken as given).  A product of two fp32 values is exact in float64 (fused or not),
    every addition rounds once, the quotient once: the restatement below does the same operations in the same order, so the
    device's float64 quotient differs from it by at most (n + 2) eps64 A', A' = sum w |y| / den, even if the device associated
    differently; the store rounds once:
        |out' - out| <= eps32 |out| + 2 (n + 2) eps64 A' + FLOOR.
    n = 1: the window's value, bits.  The clamp is exact on either side.
"""
import numpy as np

from ref_common import EPS32, EPS64, FLOOR

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------ plan
def window_starts(L, T, hop):
    assert L >= 1 and 1 <= hop <= T
    starts, s = [], 0
    while s < L - T:
        starts.append(s)
        s += hop
    return starts + [max(0, L - T)]


def window(T):
    """sin^2(pi (j + 1/2) / T), float64"""
    return np.asarray([np.sin(np.pi * (j + 0.5) / T) ** 2 for j in range(T)], F64)


def plan(lengths, T, hop, batch=1):
    """-> utt [nutt, 4], win [nwin padded to a multiple of batch, 2] (int64 here), ld, the number of real windows"""
    utt, win, col = [], [], 0
    for u, L in enumerate(lengths):
        st = window_starts(L, T, hop)
        utt.append((col, L, len(win), len(st)))
        win += [(u, s) for s in st]
        col += -(-L // 4) * 4
    n = len(win)
    while len(win) % batch:
        win.append((-1, 0))
    return np.asarray(utt, np.int64), np.asarray(win, np.int64), max(4, col), n


def rows_of(nwin_padded, batch):
    """window i -> (forward, row)"""
    return [(i // batch, i % batch) for i in range(nwin_padded)]


def cover_counts(L, T, starts):
    c = np.zeros(L, np.int64)
    for s in starts:
        c[s:min(L, s + T)] += 1
    return c


# --------------------------------------------------------------------------------------------------------------- kernels
def mel_to_windows(mels, utt, win, T):
    """mels [C, ld] fp32 -> [nwin, C, T] fp32"""
    mels = np.asarray(mels, F32)
    C = mels.shape[0]
    out = np.zeros((len(win), C, T), F32)
    for w, (u, f0) in enumerate(win):
        if u < 0:
            continue
        col0, L = utt[u][0], utt[u][1]
        for j in range(T):
            if f0 + j < L:
                out[w, :, j] = mels[:, col0 + f0 + j]
    return out


def group_sum(rows, group, G):
    """dvae_group_sum_f64 from zeroed buffers: sequential float64 sums in row order -> (sums [G, K], counts [G])"""
    rows = np.asarray(rows, F32)
    sums, counts = np.zeros((G, rows.shape[1]), F64), np.zeros(G, np.int64)
    for r, g in zip(rows, group):
        if 0 <= g < G and np.isfinite(r).all():
            sums[g] = sums[g] + r.astype(F64)
            counts[g] += 1
    return sums, counts


def window_latents(content, sums, counts, g_src, g_trg, mix, S):
    """-> (z float64 [nwin, S + Cn], tol [nwin, S + Cn]; tol 0: bits)"""
    content = np.asarray(content, F32)
    nwin, Cn = content.shape[0], content.shape[1] // 2
    z, tol = np.zeros((nwin, S + Cn), F64), np.zeros((nwin, S + Cn), F64)
    mix = float(mix)
    for w in range(nwin):
        gs, gt = int(g_src[w]), int(g_trg[w])
        if gs < 0 or gt < 0:
            continue
        a = sums[gs, :S] / F64(counts[gs])
        b = sums[gt, :S] / F64(counts[gt])
        z[w, :S] = (1.0 - mix) * a + mix * b
        if mix not in (0.0, 1.0):
            tol[w, :S] = EPS32 * np.abs(z[w, :S]) + 4 * EPS64 * (np.abs((1.0 - mix) * a) + np.abs(mix * b)) + FLOOR
        z[w, S:] = content[w, :Cn]
    return z, tol


def overlap_add(y, utt, win, w32, ld, clamp=None):
    """y [nwin, C, T] fp32, w32 [T] the fp32 window table -> dict(ref float64 [C, ld], tol, single [C, ld] bool: one window
    covers, bits; owned [C, ld] bool: written at all)"""
    y, w = np.asarray(y, F32), np.asarray(w32, F32).astype(F64)
    _, C, T = y.shape
    ref, tol = np.zeros((C, ld), F64), np.zeros((C, ld), F64)
    single, owned = np.zeros((C, ld), bool), np.zeros((C, ld), bool)
    for col0, L, win0, nw in utt:
        for t in range(L):
            cover = [k for k in range(win0, win0 + nw) if win[k][1] <= t < win[k][1] + T]
            assert cover, "a frame no window covers"
            owned[:, col0 + t] = True
            if len(cover) == 1:
                ref[:, col0 + t] = y[cover[0], :, t - win[cover[0]][1]]
                single[:, col0 + t] = True
                continue
            num, den, mag = np.zeros(C, F64), F64(0.0), np.zeros(C, F64)
            for k in cover:
                j = t - win[k][1]
                num = num + w[j] * y[k, :, j].astype(F64)
                mag = mag + w[j] * np.abs(y[k, :, j].astype(F64))
                den = den + w[j]
            ref[:, col0 + t] = num / den
            tol[:, col0 + t] = EPS32 * np.abs(num / den) + 2 * (len(cover) + 2) * EPS64 * mag / den + FLOOR
    if clamp is not None:
        ref = np.where(owned, np.minimum(np.maximum(ref, clamp[0]), clamp[1]), ref)
    return dict(ref=ref, tol=tol, single=single, owned=owned)


def close(got, res):
    """Predicate of the comparison the GPU suite makes: bits where one window covers, the bound elsewhere, owned columns only."""
    got = np.asarray(got, F32)
    o, s = res["owned"], res["single"]
    if not np.array_equal(got[s].view(np.uint32), res["ref"][s].astype(F32).view(np.uint32)):
        return False
    m = o & ~s
    with np.errstate(invalid="ignore"):
        return bool((np.abs(got[m].astype(F64) - res["ref"][m]) <= res["tol"][m]).all())


def latents_close(got, z, tol):
    got = np.asarray(got, F32)
    exact = tol == 0
    if not np.array_equal(got[exact].view(np.uint32), z[exact].astype(F32).view(np.uint32)):
        return False
    with np.errstate(invalid="ignore"):
        return bool((np.abs(got[~exact].astype(F64) - z[~exact]) <= tol[~exact]).all())


# ----------------------------------------------------------------------------------------------------------------- cases
def _batch_with_padding(nwin):
    return next(b for b in (4, 3, 5, 7) if nwin % b)


def cases():
    """The smallest shapes that can still go wrong: C in {1, 3}, T in {4, 8}, hop in {1, T/2, T - 1, T}, L over {1, T - 1, T,
    T + 1, 2T, 2T + 3}, three utterances in one packed buffer, at least one padding window in the list."""
    out = []
    for C in (1, 3):
        for T in (4, 8):
            for hop in (1, T // 2, T - 1, T):
                for lengths in ((1, T + 1, 2 * T + 3), (T - 1, 2 * T, T)):
                    nwin = sum(len(window_starts(L, T, hop)) for L in lengths)
                    out.append(dict(C=C, T=T, hop=hop, lengths=lengths, batch=_batch_with_padding(nwin)))
    return out


CASES = cases()
GRID = [(L, T, hop) for T in (4, 8) for hop in (1, T // 2, T - 1, T) for L in (1, T - 1, T, T + 1, 2 * T, 2 * T + 3)]


def case_id(c):
    return "C{C}-T{T}-hop{hop}-L{0}".format("_".join(map(str, c["lengths"])), **c)


def case_data(c, seed=0):
    """utt, win, ld, nwin, mels [C, ld] fp32 in [0, 1] (NaN in the columns no utterance owns: a read of one shows), y [nwin
    padded, C, T] fp32 decoded-window stand-ins in [-0.2, 1.2] (so that the clamp bites), w32."""
    rng = np.random.RandomState(1000 * seed + 97 * c["C"] + 13 * c["T"] + c["hop"] + sum(c["lengths"]))
    utt, win, ld, nwin = plan(c["lengths"], c["T"], c["hop"], c["batch"])
    assert len(win) > nwin, "every case holds a padding window"
    mels = np.full((c["C"], ld), np.nan, F32)
    for col0, L, _, _ in utt:
        mels[:, col0:col0 + L] = rng.rand(c["C"], L).astype(F32)
    y = (rng.rand(len(win), c["C"], c["T"]) * 1.4 - 0.2).astype(F32)
    return dict(utt=utt, win=win, ld=ld, nwin=nwin, mels=mels, y=y, w32=window(c["T"]).astype(F32))


def latent_case(seed=0):
    """G = 3 style groups over eight windows, one of them a single window, one padding window at the end; S = 2 (K = 4),
    Cn = 3.  g_src: the window's own group; g_trg: another one."""
    rng = np.random.RandomState(seed + 5)
    S, Cn, G = 2, 3, 3
    group = np.asarray([0, 0, 2, 0, 1, 2, 0, -1], np.int32)
    style = rng.randn(8, 2 * S).astype(F32)
    content = rng.randn(8, 2 * Cn).astype(F32)
    sums, counts = group_sum(style, group, G)
    g_trg = np.where(group >= 0, (group + 1) % G, -1).astype(np.int32)
    return dict(S=S, Cn=Cn, G=G, style=style, content=content, sums=sums, counts=counts, g_src=group, g_trg=g_trg)
