"""F0 tracking and the log-F0 RMSE along the MCD alignment (dvae_amd.evaluate) on the host: a float64
restatement of the Viterbi pass over the autocorrelation lags (local score, octave cost, octave-jump cost, runs of voiced
frames, parabolic refinement) built on test_mcd.frames_ref and the `ev` tables, against the true pitch of tones and chirps,
against the frame-wise arg-max it replaces and against a brute-force enumeration; the DTW restatement with a payload
against test_mcd.dtw_ref and a traced-back path; and the CLI's flag.
The float64 restatements here are also the yardsticks of tests/test_hip_f0.py."""
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dvae_amd  # noqa: E402,F401
from dvae_amd import evaluate as ev  # noqa: E402
from test_mcd import dtw_ref, frames_ref, harmonic  # noqa: E402


# ----------------------------------------------------------------------------------------- float64 restatements
def autocorr_ref(wav):
    """[M, 207] float32: r(0), r(20..225) of every frame, computed in float64 and rounded as the GPU buffer is"""
    P = np.abs(np.fft.rfft(frames_ref(wav), n=ev.FFT_SIZE, axis=1)) ** 2
    return np.fft.irfft(P, n=ev.FFT_SIZE, axis=1)[:, ev.lags()].astype(np.float32)


def gain32():
    """the window gain as the device holds it"""
    return ev.window_gain().astype(np.float32)


def voiced_ref(r, gain):
    """the voicing rule of §4.6 on r [M, 207]"""
    r = r.astype(np.float64)
    r0 = r[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        peak = np.where(r0 > 0, np.max(r[:, 1:] * gain[None, 1:], axis=1) / np.where(r0 > 0, r0, 1.0), 0.0)
    return (r0 > 0) & (r0 >= ev.VOICED_REL_POWER * r0.max()) & (peak >= ev.VOICED_PEAK)


def local_scores(r, gain, octave_cost=ev.OCTAVE_COST):
    """s [K, 206] float64 of voiced frames r [K, 207] (fp32): r * gain / r(0) - oct, every operation rounded once"""
    l2 = ev.f0_tables()[0]
    q = r[:, 1:].astype(np.float64) * gain[None, 1:].astype(np.float64)
    return q / r[:, :1].astype(np.float64) - octave_cost * (l2 - l2[0])


def viterbi_run(s, l2, jump_cost):
    """one run: s [K, S] -> (states [K], D of the last frame [S]); the first maximal predecessor / final state on a tie"""
    K, S = s.shape
    T = jump_cost * np.abs(l2[:, None] - l2[None, :])          # [j, i]
    D = s[0].copy()
    back = np.zeros((K, S), np.int64)
    for k in range(1, K):
        cand = D[None, :] - T
        back[k] = np.argmax(cand, axis=1)
        D = s[k] + cand[np.arange(S), back[k]]
    st = np.zeros(K, np.int64)
    st[-1] = int(np.argmax(D))
    for k in range(K - 1, 0, -1):
        st[k - 1] = back[k, st[k]]
    return st, D


def runs_of(voiced):
    """[(first, last)] of every maximal run of voiced frames"""
    v = np.concatenate([[0], np.asarray(voiced).astype(np.int8), [0]])
    d = np.diff(v)
    return list(zip(np.nonzero(d == 1)[0], np.nonzero(d == -1)[0] - 1))


def refine(r_row, gain, j):
    """f0 in Hz (float32) of state j on one frame: the parabolic vertex of q = r * gain around the lag"""
    delta = 0.0
    if 0 < j < ev.F0_STATES - 1:
        q = r_row[j:j + 3].astype(np.float64) * gain[j:j + 3].astype(np.float64)     # columns 1 + (j-1 .. j+1)
        den = q[0] - 2.0 * q[1] + q[2]
        if den < 0:
            delta = min(0.5, max(-0.5, 0.5 * (q[0] - q[2]) / den))
    return np.float32(ev.SAMPLE_RATE / ((ev.LAG_MIN + j) + delta))


def track_ref(r, gain, voiced, octave_cost=ev.OCTAVE_COST, jump_cost=ev.JUMP_COST):
    """the whole tracker on one utterance: r [M, 207] fp32, voiced [M] -> dict(state [M] (-1 unvoiced), f0 [M] float32,
    margin [runs]: best minus second-best of each run's last D, objective [runs])"""
    l2 = ev.f0_tables()[0]
    M = r.shape[0]
    state = np.full(M, -1, np.int64)
    f0 = np.zeros(M, np.float32)
    margin, objective = [], []
    for a, b in runs_of(voiced):
        s = local_scores(r[a:b + 1], gain, octave_cost)
        st, D = viterbi_run(s, l2, jump_cost)
        state[a:b + 1] = st
        top = np.sort(D)[::-1]
        margin.append(top[0] - top[1])
        objective.append(path_objective(s, l2, st, jump_cost))
        for k in range(a, b + 1):
            f0[k] = refine(r[k], gain, state[k])
    return dict(state=state, f0=f0, margin=np.array(margin), objective=np.array(objective))


def path_objective(s, l2, st, jump_cost=ev.JUMP_COST):
    """the quantity the Viterbi pass maximises, of a given state path over one run"""
    st = np.asarray(st)
    return float(np.sum(s[np.arange(len(st)), st]) - jump_cost * np.sum(np.abs(np.diff(l2[st]))))


def dtw_payload_ref(x, y, lx, ly):
    """test_mcd.dtw_ref with the sum of (lx[i] - ly[j])^2 over the path's cells carried the way the length is
    -> (cost, length, sse); (nan, 0, nan) when a side is empty"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    lx, ly = np.asarray(lx, np.float64).reshape(-1), np.asarray(ly, np.float64).reshape(-1)
    N, M = x.shape[0], y.shape[0]
    if N == 0 or M == 0:
        return float("nan"), 0, float("nan")
    inf = np.inf
    c1, c2 = np.full(N, inf), np.full(N, inf)
    l1, l2 = np.zeros(N, np.int64), np.zeros(N, np.int64)
    p1, p2 = np.zeros(N), np.zeros(N)
    for d in range(N + M - 1):
        i = np.arange(max(0, d - M + 1), min(N - 1, d) + 1)
        j = d - i
        dd = np.sqrt(np.sum((x[i] - y[j]) ** 2, axis=1))
        e = (lx[i] - ly[j]) ** 2
        im = np.maximum(i - 1, 0)
        cand = np.stack([np.where(i > 0, c1[im], inf), np.where(j > 0, c1[i], inf),
                         np.where((i > 0) & (j > 0), c2[im], inf)])
        k = np.argmin(cand, axis=0)
        cols = np.arange(len(i))
        best = cand[k, cols]
        blen = np.stack([l1[im], l1[i], l2[im]])[k, cols]
        bpay = np.stack([p1[im], p1[i], p2[im]])[k, cols]
        start = (i == 0) & (j == 0)
        nc, nl, npay = np.full(N, inf), np.zeros(N, np.int64), np.zeros(N)
        nc[i] = np.where(start, dd, dd + best)
        nl[i] = np.where(start, 1, blen + 1)
        npay[i] = np.where(start, e, bpay + e)
        c2, l2, p2, c1, l1, p1 = c1, l1, p1, nc, nl, npay
    return float(c1[N - 1]), int(l1[N - 1]), float(p1[N - 1])


def dtw_traceback(x, y):
    """the textbook matrix, cell by cell, then the path walked back from the corner: [(i, j)] from (0, 0)"""
    N, M = len(x), len(y)
    D = np.full((N, M), np.inf)
    prev = {}
    for i in range(N):
        for j in range(M):
            d = float(np.sqrt(np.sum((np.asarray(x[i], np.float64) - np.asarray(y[j], np.float64)) ** 2)))
            if i == 0 and j == 0:
                D[i, j] = d
                continue
            cands = [((i - 1, j), D[i - 1, j] if i > 0 else np.inf), ((i, j - 1), D[i, j - 1] if j > 0 else np.inf),
                     ((i - 1, j - 1), D[i - 1, j - 1] if i > 0 and j > 0 else np.inf)]
            cell, best = min(cands, key=lambda t: t[1])
            D[i, j] = d + best
            prev[i, j] = cell
    path = [(N - 1, M - 1)]
    while path[-1] != (0, 0):
        path.append(prev[path[-1]])
    return path[::-1]


# ---------------------------------------------------------------------------------------------------- the signals
def chirp(n, f_from, f_to, amplitudes=None, snr_db=30.0, seed=0, sr=16000):
    """a harmonic linear chirp (amplitudes default 1/k, 8 harmonics) plus white noise snr_db below it
    -> (float32 signal, the instantaneous fundamental at every sample)"""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / sr
    T = n / sr
    amplitudes = [1.0 / k for k in range(1, 9)] if amplitudes is None else amplitudes
    phase = 2 * np.pi * (f_from * t + (f_to - f_from) * t ** 2 / (2 * T))
    x = sum(a * np.sin(k * phase + rs.uniform(0, 2 * np.pi)) for k, a in enumerate(amplitudes, start=1))
    x = 0.3 * x / np.sqrt(np.mean(x ** 2))
    x = x + rs.randn(n) * np.sqrt(np.mean(x ** 2)) * 10 ** (-snr_db / 20)
    return x.astype(np.float32), f_from + (f_to - f_from) * t / T


TONES = (71.5, 100.0, 120.0, 220.0, 400.0, 790.0)
OCTAVE_PRONE = (220.0, 400.0, 790.0)


def pitch_signals():
    """[(name, signal, true f0 of every frame)]: the tones and chirps of DESIGN.md §4.7"""
    out = []
    for f in TONES:
        x = harmonic(8000, f, seed=int(f))
        out.append((f"tone {f}", x, np.full(ev.frame_count(len(x)), f)))
    for name, (a, b, amps, snr, seed) in {
            "chirp 100-300": (100.0, 300.0, None, 30.0, 1), "chirp 400-90": (400.0, 90.0, None, 30.0, 2),
            "chirp 120-240 even": (120.0, 240.0, [0.1, 1, 0.1, 0.8, 0.05, 0.5, 0.02, 0.3], 30.0, 3),
            "chirp 150-200 10 dB": (150.0, 200.0, None, 10.0, 4)}.items():
        x, inst = chirp(16000, a, b, amps, snr, seed)
        centre = np.minimum(np.arange(ev.frame_count(len(x))) * ev.HOP, len(x) - 1)
        out.append((name, x, inst[centre]))
    return out


def cents(f, truth):
    return 1200.0 * np.abs(np.log2(np.asarray(f, np.float64) / truth))


@pytest.fixture(scope="module")
def tracked():
    """every signal once: (name, truth, r, voiced, the tracker's result)"""
    g = gain32()
    out = []
    for name, x, truth in pitch_signals():
        r = autocorr_ref(x)
        v = voiced_ref(r, g)
        out.append((name, truth, r, v, track_ref(r, g, v)))
    return out


# ------------------------------------------------------------------------------------------------------- tracking
def test_tables():
    l2, octc = ev.f0_tables()
    assert ev.F0_STATES == 206 and l2.shape == octc.shape == (206,) and l2.dtype == np.float64
    assert l2[0] == np.log2(20.0) and l2[-1] == np.log2(225.0) and octc[0] == 0.0
    assert np.array_equal(octc, ev.OCTAVE_COST * (l2 - l2[0]))
    assert ev.OCTAVE_COST == 0.01 and ev.JUMP_COST == 0.35


def test_tracker_follows_tones_and_chirps_where_the_argmax_does_not(tracked):
    g = gain32()
    for name, truth, r, v, res in tracked:
        inner = np.nonzero(v)[0]
        inner = inner[(inner >= 4) & (inner < len(v) - 4)]
        assert inner.size >= 0.9 * (len(v) - 8), (name, inner.size)
        err = cents(res["f0"][inner], truth[inner])
        print(f"{name}: max error {err.max():.2f} cents over {inner.size} frames")
        assert err.max() <= 50.0, (name, err.max())
        assert not np.any(err > 600.0), name
        if name in [f"tone {f}" for f in OCTAVE_PRONE]:
            # what the Viterbi pass is for: the frame-wise arg-max of the normalised autocorrelation is octaves off
            q = r[inner, 1:].astype(np.float64) * g[None, 1:] / r[inner, :1]
            am = ev.SAMPLE_RATE / (ev.LAG_MIN + np.argmax(q, axis=1))
            off = np.mean(cents(am, truth[inner]) > 600.0)
            print(f"{name}: arg-max more than 600 cents off on {100 * off:.0f} % of the frames")
            assert off >= 0.5, (name, off)


def test_without_costs_the_tracker_is_the_argmax(tracked):
    g = gain32()
    for name, truth, r, v, _ in tracked[3:8]:
        res = track_ref(r, g, v, octave_cost=0.0, jump_cost=0.0)
        idx = np.nonzero(v)[0]
        q = r[idx, 1:].astype(np.float64) * g[None, 1:].astype(np.float64) / r[idx, :1].astype(np.float64)
        assert np.array_equal(res["state"][idx], np.argmax(q, axis=1)), name
        assert np.all(res["state"][~v] == -1) and np.all(res["f0"][~v] == 0.0)


def test_recurrence_matches_brute_force():
    rs = np.random.RandomState(5)
    l2 = np.log2(np.array([20.0, 31.0, 40.0, 80.0, 160.0]))
    for trial in range(20):
        s = rs.uniform(0.0, 1.0, (4, 5))
        st, D = viterbi_run(s, l2, ev.JUMP_COST)
        paths = list(itertools.product(range(5), repeat=4))
        scores = np.array([path_objective(s, l2, p) for p in paths])
        assert tuple(st) == paths[int(np.argmax(scores))], trial
        assert abs(D.max() - scores.max()) <= 1e-14 and abs(path_objective(s, l2, st) - scores.max()) <= 1e-14


def test_ties_go_to_the_first_state():
    l2 = np.log2(np.array([20.0, 40.0, 80.0]))
    st, D = viterbi_run(np.zeros((3, 3)), l2, 0.0)
    assert list(st) == [0, 0, 0] and np.all(D == 0.0)
    st, _ = viterbi_run(np.array([[0.0, 1.0, 1.0], [0.0, 0.0, 0.0]]), l2, 0.0)
    assert list(st) == [1, 0]                 # last frame: the first of the tied D; before it: the first maximal i


def test_runs_are_tracked_on_their_own():
    g = gain32()
    x = np.concatenate([harmonic(4000, 120.0, seed=1), np.zeros(2400, np.float32), harmonic(4000, 300.0, seed=2)])
    r = autocorr_ref(x)
    v = voiced_ref(r, g)
    runs = runs_of(v)
    assert len(runs) == 2
    res = track_ref(r, g, v)
    for a, b in runs:
        alone = track_ref(r[a:b + 1], g, np.ones(b - a + 1, bool))
        assert np.array_equal(alone["state"], res["state"][a:b + 1])
    # the second run starts from its own local score: carrying the first run's D over the silence would pull its first
    # frames towards 120 Hz's lag
    a, b = runs[1]
    assert np.all(cents(res["f0"][a + 4:b - 3], 300.0) < 50.0)
    assert np.all(res["f0"][~v] == 0.0) and np.all(res["f0"][v] > 0.0)


def test_refinement_edges_and_clamp():
    g = np.ones(207, np.float32)
    row = np.zeros(207, np.float32)
    row[0] = 1.0
    assert refine(row, g, 0) == np.float32(16000 / 20) and refine(row, g, 205) == np.float32(16000 / 225)
    row[1 + 100 - 1:1 + 100 + 2] = [0.5, 1.0, 0.5]                     # symmetric peak: no shift
    assert refine(row, g, 100) == np.float32(16000 / 120)
    row[1 + 100 - 1:1 + 100 + 2] = [0.9, 1.0, 0.5]                     # vertex towards the larger neighbour (a shorter lag)
    assert 16000 / 120 < refine(row, g, 100) <= np.float32(16000 / 119.5)
    row[1 + 100 - 1:1 + 100 + 2] = [1.0, 1.0, 0.0]                     # vertex at -0.5: the clamp's edge
    assert refine(row, g, 100) == np.float32(16000 / 119.5)
    row[1 + 100 - 1:1 + 100 + 2] = [0.5, 0.2, 0.5]                     # convex: left alone
    assert refine(row, g, 100) == np.float32(16000 / 120)


# ------------------------------------------------------------------------------------------------------------- DTW
@pytest.mark.parametrize("N,M", [(1, 1), (1, 7), (7, 1), (5, 9), (9, 5), (7, 9), (6, 6)])
def test_payload_dtw_matches_dtw_ref_and_a_traced_back_path(N, M):
    rs = np.random.RandomState(N * 31 + M)
    for x, y in ((rs.randn(N, 24), rs.randn(M, 24)), (rs.randint(0, 2, (N, 3)), rs.randint(0, 2, (M, 3)))):
        lx, ly = rs.uniform(4.0, 6.5, N), rs.uniform(4.0, 6.5, M)
        c, l, sse = dtw_payload_ref(x, y, lx, ly)
        c0, l0 = dtw_ref(x, y)
        assert c == c0 and l == l0
        path = dtw_traceback(x, y)
        assert len(path) == l
        want = sum((lx[i] - ly[j]) ** 2 for i, j in path)
        assert abs(sse - want) <= 1e-12 * max(1.0, want), (sse, want)


def test_payload_dtw_empty_side_and_identity():
    c, l, sse = dtw_payload_ref(np.zeros((0, 24)), np.zeros((3, 24)), np.zeros(0), np.zeros(3))
    assert np.isnan(c) and l == 0 and np.isnan(sse)
    x = np.random.RandomState(6).randn(30, 24)
    lf = np.random.RandomState(7).uniform(4, 6, 30)
    assert dtw_payload_ref(x, x, lf, lf) == (0.0, 30, 0.0)
    assert ev.lf0_rmse_from([8.0], [2])[0] == 2.0 and np.isnan(ev.lf0_rmse_from([np.nan], [0])[0])
    assert np.isclose(ev.CENTS_PER_NAT * np.log(2.0), 1200.0, rtol=1e-15)
    m, s = ev.lf0_stats(np.log([100.0, 200.0]))
    assert np.isclose(np.exp(m), np.sqrt(100.0 * 200.0)) and np.isclose(s, np.log(2.0) / 2)
    assert all(np.isnan(v) for v in ev.lf0_stats([]))


# ------------------------------------------------------------------------------------------------------------- CLI
def test_cli_flag_defaults_to_off():
    assert ev._parse(["conv", "ref"]).f0 is False
    assert ev._parse(["conv", "ref", "--f0"]).f0 is True
    assert ev._parse(["conv", "ref", "--f0", "--json", "x.json"]).json.name == "x.json"
