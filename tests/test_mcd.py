"""Mel-cepstral distortion (dvae_amd.evaluate) on the host: the float64 tables against the published
definitions they restate (pysptk.sp2mc = irfft -> c[0] / 2 -> SPTK freqt; the autocorrelation of the zero-padded frame),
the voicing rule, a numpy DTW with the kernel's tie order against a brute-force recursion, and the CLI's pairing.
The float64 restatements here are also the yardsticks of tests/test_hip_mcd.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dvae_amd  # noqa: E402,F401
from dvae_amd import evaluate as ev  # noqa: E402


# ----------------------------------------------------------------------------------------- float64 restatements
def freqt_ref(c, order, alpha):
    """SPTK freqt as published (freqt.c), vectorised over the leading axes of c [..., m1 + 1]"""
    c = np.asarray(c, dtype=np.float64)
    b = 1.0 - alpha * alpha
    g = np.zeros(c.shape[:-1] + (order + 1,))
    for i in range(c.shape[-1] - 1, -1, -1):
        d = g.copy()
        g[..., 0] = c[..., i] + alpha * d[..., 0]
        if order >= 1:
            g[..., 1] = b * d[..., 0] + alpha * d[..., 1]
        for j in range(2, order + 1):
            g[..., j] = d[..., j - 1] + alpha * (d[..., j] - g[..., j - 1])
    return g


def sp2mc_ref(log_power, order=ev.ORDER, alpha=ev.ALPHA):
    """pysptk.sp2mc on a log power spectrum [..., 513]: irfft, c[0] / 2, freqt"""
    c = np.fft.irfft(log_power, n=ev.FFT_SIZE, axis=-1)
    c[..., 0] /= 2.0
    return freqt_ref(c, order, alpha)


def frames_ref(wav):
    """[M, 512] float64: frame k = periodic Hann x the samples 80 k - 256 .. 80 k + 255 (zero outside the signal)"""
    x = np.asarray(wav, dtype=np.float64)
    n = x.shape[0]
    M = ev.frame_count(n)
    idx = np.arange(M)[:, None] * ev.HOP + np.arange(ev.FRAME)[None, :] - ev.FRAME // 2
    f = np.where((idx >= 0) & (idx < n), x[np.clip(idx, 0, max(0, n - 1))] if n else 0.0, 0.0)
    return f * ev.hann_periodic()[None, :]


def features_ref(wav):
    """the feature pass in float64 -> dict(mc [M, 36], voiced [M], peak [M], r0 [M])"""
    P = np.abs(np.fft.rfft(frames_ref(wav), n=ev.FFT_SIZE, axis=1)) ** 2
    mc = sp2mc_ref(np.log(np.maximum(P, ev.POWER_FLOOR)))
    r = np.fft.irfft(P, n=ev.FFT_SIZE, axis=1)[:, ev.lags()]
    r0 = r[:, 0]
    gain = ev.window_gain()
    with np.errstate(invalid="ignore", divide="ignore"):
        peak = np.where(r0 > 0, np.max(r[:, 1:] * gain[None, 1:], axis=1) / np.where(r0 > 0, r0, 1.0), 0.0)
    voiced = (r0 > 0) & (r0 >= ev.VOICED_REL_POWER * r0.max()) & (peak >= ev.VOICED_PEAK)
    return dict(mc=mc, voiced=voiced, peak=peak, r0=r0)


def dtw_ref(x, y):
    """exact DTW in float64, anti-diagonal vectorised: (i-1,j), (i,j-1), (i-1,j-1) in that order of preference on a tie
    -> (cost, path length); (nan, 0) when a side is empty"""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    N, M = x.shape[0], y.shape[0]
    if N == 0 or M == 0:
        return float("nan"), 0
    inf = np.inf
    c1, c2 = np.full(N, inf), np.full(N, inf)          # diagonals d-1, d-2, indexed by i
    l1, l2 = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for d in range(N + M - 1):
        i = np.arange(max(0, d - M + 1), min(N - 1, d) + 1)
        j = d - i
        dd = np.sqrt(np.sum((x[i] - y[j]) ** 2, axis=1))
        up = np.where(i > 0, c1[np.maximum(i - 1, 0)], inf)
        lup = np.where(i > 0, l1[np.maximum(i - 1, 0)], 0)
        left = np.where(j > 0, c1[i], inf)
        dg = np.where((i > 0) & (j > 0), c2[np.maximum(i - 1, 0)], inf)
        ldg = l2[np.maximum(i - 1, 0)]
        cand = np.stack([up, left, dg])
        k = np.argmin(cand, axis=0)                      # the first minimum
        best = cand[k, np.arange(len(i))]
        blen = np.stack([lup, l1[i], ldg])[k, np.arange(len(i))]
        start = (i == 0) & (j == 0)
        nc, nl = np.full(N, inf), np.zeros(N, np.int64)
        nc[i] = np.where(start, dd, dd + best)
        nl[i] = np.where(start, 1, blen + 1)
        c2, l2, c1, l1 = c1, l1, nc, nl
    return float(c1[N - 1]), int(l1[N - 1])


def dtw_brute(x, y):
    """the textbook recursion, cell by cell, min over (cost, predecessor) tuples in fastdtw's order"""
    N, M = len(x), len(y)
    D = {}
    for i in range(N):
        for j in range(M):
            d = float(np.sqrt(np.sum((np.asarray(x[i], np.float64) - np.asarray(y[j], np.float64)) ** 2)))
            if i == 0 and j == 0:
                D[i, j] = (d, 1)
                continue
            cands = [D.get((i - 1, j), (np.inf, 0)), D.get((i, j - 1), (np.inf, 0)), D.get((i - 1, j - 1), (np.inf, 0))]
            best = min(cands, key=lambda t: t[0])
            D[i, j] = (d + best[0], best[1] + 1)
    return D[N - 1, M - 1]


def harmonic(n, f0, sr=16000, seed=0, snr_db=30.0, harmonics=8):
    """a harmonic tone (1/k amplitudes) plus white noise snr_db below it, float32"""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / sr
    x = sum(np.sin(2 * np.pi * k * f0 * t + rs.uniform(0, 2 * np.pi)) / k for k in range(1, harmonics + 1)
            if k * f0 < sr / 2)
    x = 0.3 * x / np.sqrt(np.mean(x ** 2))
    x = x + rs.randn(n) * np.sqrt(np.mean(x ** 2)) * 10 ** (-snr_db / 20)
    return x.astype(np.float32)


def write_pcm16(path, x, sr=16000):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes((np.clip(np.asarray(x), -1, 1) * 32767).astype("<i2").tobytes())


# --------------------------------------------------------------------------------------------------------- tables
def test_sp2mc_matrix_is_the_published_recursion():
    rs = np.random.RandomState(0)
    S = ev.sp2mc_matrix()
    assert S.shape == (ev.ORDER + 1, ev.FFT_SIZE // 2 + 1)
    lp = rs.uniform(-20.0, 10.0, (6, ev.FFT_SIZE // 2 + 1))
    lp[0] = np.log(np.maximum(np.abs(np.fft.rfft(rs.randn(512), ev.FFT_SIZE)) ** 2, ev.POWER_FLOOR))
    got, ref = lp @ S.T, sp2mc_ref(lp)
    assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref))), np.max(np.abs(got - ref))


def test_freqt_with_zero_alpha_is_the_truncation():
    c = np.random.RandomState(1).randn(3, 40)
    assert np.allclose(freqt_ref(c, 35, 0.0), c[:, :36], rtol=0, atol=1e-15)
    assert np.allclose(ev.freqt_matrix(39, 35, 0.0), np.eye(40)[:36], rtol=0, atol=0)


def test_lag_basis_is_the_autocorrelation_of_the_padded_frame():
    rs = np.random.RandomState(2)
    L = ev.lag_basis()
    lags = ev.lags()
    assert lags[0] == 0 and lags[1] == 20 and lags[-1] == 225 and L.shape == (len(lags), ev.FFT_SIZE // 2 + 1)
    for trial in range(3):
        f = ev.hann_periodic() * rs.randn(ev.FRAME)
        P = np.abs(np.fft.rfft(f, ev.FFT_SIZE)) ** 2
        full = np.correlate(f, f, mode="full")              # lag 0 at index FRAME - 1
        ref = full[ev.FRAME - 1 + lags]
        assert np.max(np.abs(L @ P - ref)) <= 1e-10 * ref[0]
    w = ev.hann_periodic()
    g = ev.window_gain()
    assert g[0] == 1.0 and np.all(g[1:] > 1.0)
    assert np.isclose(g[5], np.dot(w, w) / np.dot(w[:-lags[5]], w[lags[5]:]), rtol=1e-14)


def test_frames_are_centred_every_5_ms():
    n = 1234
    x = np.zeros(n, np.float32)
    x[400] = 1.0                                              # sample 400 = the centre of frame 5
    f = frames_ref(x)
    assert f.shape == (n // 80 + 1, 512) and ev.frame_count(n) == n // 80 + 1
    assert f[5, 256] == 1.0 and f[5].sum() == 1.0


# --------------------------------------------------------------------------------------------------------- voicing
def test_voicing_rule_separates_tones_from_noise():
    rs = np.random.RandomState(3)
    noise = features_ref(rs.randn(16000).astype(np.float32))
    assert noise["voiced"].mean() == 0.0, noise["peak"].max()
    assert noise["peak"].max() < 0.40
    for f0 in (71.0, 120.0, 400.0, 800.0):
        fr = features_ref(harmonic(16000, f0, seed=int(f0)))
        inner = fr["voiced"][4:-4]                        # frames whose window lies inside the signal
        assert inner.all(), (f0, fr["peak"][4:-4].min())
    silent = features_ref(np.zeros(4000, np.float32))
    assert not silent["voiced"].any()


# ------------------------------------------------------------------------------------------------------------- DTW
@pytest.mark.parametrize("N,M", [(1, 1), (1, 7), (7, 1), (5, 9), (9, 5), (12, 12)])
def test_dtw_restatement_matches_brute_force(N, M):
    rs = np.random.RandomState(N * 31 + M)
    for feats in (rs.randn(N, 24), rs.randn(M, 24)), (rs.randint(0, 2, (N, 3)), rs.randint(0, 2, (M, 3))):
        x, y = feats
        c, l = dtw_ref(x, y)
        cb, lb = dtw_brute(x, y)
        assert l == lb and abs(c - cb) <= 1e-12 * max(1.0, cb), (c, cb, l, lb)


def test_dtw_tie_order_is_fastdtws():
    assert dtw_ref(np.zeros((2, 1)), np.zeros((1, 1))) == (0.0, 2)
    # 2 x 2 of zeros: D(1,1) takes the first of D(0,1) = (0, len 2), D(1,0), D(0,0) = (0, len 1): length 3, not 2
    assert dtw_ref(np.zeros((2, 1)), np.zeros((2, 1))) == (0.0, 3)
    assert dtw_brute(np.zeros((2, 1)), np.zeros((2, 1))) == (0.0, 3)


def test_mcd_of_a_sequence_against_itself_is_zero():
    x = np.random.RandomState(4).randn(50, 24)
    c, l = dtw_ref(x, x)
    assert c == 0.0 and l == 50
    assert ev.mcd_from([c], [l])[0] == 0.0
    assert np.isnan(ev.mcd_from([np.nan], [0])[0])
    assert np.isclose(ev.mcd_from([3.0], [2])[0], 10 / np.log(10) * np.sqrt(2) * 1.5, rtol=1e-15)


# ------------------------------------------------------------------------------------------------------------- CLI
def test_pairing_and_unmatched(tmp_path):
    from pathlib import Path
    assert ev.utterance_id("convert_p225_to_p226_003.wav") == "003"
    assert ev.utterance_id(Path("/x/p226_003.wav")) == "003"
    cv = [Path(f"convert_p225_to_p226_{u}.wav") for u in ("001", "002", "007")] + [Path("other_p225_to_p226_001.wav")]
    rf = [Path(f"p226_{u}.wav") for u in ("001", "002", "003")]
    pairs, un_c, un_r = ev.pair_files(cv, rf)
    assert [(u, c.name, r.name) for u, c, r in pairs] == [("001", "convert_p225_to_p226_001.wav", "p226_001.wav"),
                                                         ("002", "convert_p225_to_p226_002.wav", "p226_002.wav")]
    assert [p.name for p in un_c] == ["convert_p225_to_p226_007.wav", "other_p225_to_p226_001.wav"]
    assert [p.name for p in un_r] == ["p226_003.wav"]


def test_cli_without_a_match_exits_nonzero(tmp_path):
    cdir, rdir = tmp_path / "conv", tmp_path / "ref"
    cdir.mkdir()
    rdir.mkdir()
    write_pcm16(cdir / "convert_p225_to_p226_001.wav", np.zeros(800))
    write_pcm16(rdir / "p226_002.wav", np.zeros(800))
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "dvae_amd.evaluate", str(cdir), str(rdir)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 1, p.stdout + p.stderr
    assert "no converted file" in p.stderr
    res = json.loads((cdir / "mcd.json").read_text())
    assert res["pairs"] == [] and res["unmatched"]["converted"][0].endswith("convert_p225_to_p226_001.wav")
    assert res["unmatched"]["reference"][0].endswith("p226_002.wav")
