"""Griffin-Lim inverse of the mel front-end (frontend.MelInverter).  CPU: the host-side tables of `frontend.inverse_tables`
and a float64 numpy restatement of the whole inverse (denormalise -> clamped pinv + projected gradient -> fast
Griffin-Lim on the lws framing), which tests/test_hip_griffinlim.py holds the GPU to.  The restatement takes a dtype so
that the GPU's distance from float64 can be compared with what float32 arithmetic alone costs."""
import numpy as np

from oracle import mel_ref

FS, HOP, NM = mel_ref.FFT_SIZE, mel_ref.HOP_SIZE, mel_ref.NUM_MELS


def tables():
    import dvae_amd  # noqa: F401
    from dvae_amd.frontend import inverse_tables
    return inverse_tables(mel_ref.SAMPLE_RATE, FS, HOP, NM, mel_ref.FMIN, mel_ref.FMAX)


def signal(n, seed):
    """the synthetic test signal of tests/test_frontend.py"""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / 16000.0
    return (0.25 * np.sin(2 * np.pi * (200 + 37 * seed) * t) + 0.1 * np.sin(2 * np.pi * 2500 * t * (1 + 0.3 * t))
            + 0.03 * rs.standard_normal(n)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the restatement
def amplitude(mel):
    """[80, M] normalised -> [M, 80] mel amplitude (inverse of normalize / amp_to_db - ref_level_db)"""
    db = mel_ref.denormalize(np.asarray(mel, dtype=np.float64)) + mel_ref.REF_LEVEL_DB
    return (10.0 ** (db / 20.0)).T


def linear_magnitude(mel, iters=200, tb=None):
    """-> X [M, nbp] >= 0: max(0, A pinv^T), then `iters` projected-gradient steps"""
    tb = tb or tables()
    A = amplitude(mel)
    W = tb["mel_basis"]
    X = np.maximum(0.0, A @ tb["pinv"].T)
    for _ in range(iters):
        X = np.maximum(0.0, X - tb["step"] * ((X @ W.T - A) @ W))
    return X


def residual(X, mel, tb=None):
    """per frame ||M X - A|| / ||A||"""
    tb = tb or tables()
    A = amplitude(mel)
    X = np.asarray(X, np.float64)
    W = tb["mel_basis"][:, :X.shape[1]]
    return np.linalg.norm(X @ W.T - A, axis=1) / np.linalg.norm(A, axis=1)


def _ola(y, w, n, dtype):
    M = y.shape[0]
    s = np.zeros((M - 1) * HOP + FS, dtype=dtype)
    for m in range(M):
        s[m * HOP:m * HOP + FS] += w * y[m]
    return s[FS - HOP:FS - HOP + n]


def _frames(s, w, M):
    x = np.concatenate((np.zeros(FS - HOP, s.dtype), s, np.zeros(FS, s.dtype)))
    idx = np.arange(FS)[None, :] + HOP * np.arange(M)[:, None]
    return x[idx] * w[None, :]


def griffin_lim(S, phase, n_iter, momentum=0.99, dtype=np.float64, tb=None):
    """S [M, nb or nbp] magnitude, phase [M, nb] radians or None (zero phase) -> waveform of (M - 3) * hop samples.
    Fast Griffin-Lim (librosa.griffinlim) with STFT / iSTFT of the lws framing as one-sided DFT matrices."""
    from dvae_amd.frontend import dft_basis
    tb = tb or tables()
    nb, nbp = tb["nb"], tb["nbp"]
    M = S.shape[0]
    n = (M - FS // HOP + 1) * HOP
    w = tb["window"].astype(dtype)
    fwd, inv = dft_basis(FS, nbp).astype(dtype), tb["inv_basis"].astype(dtype)
    Sp = np.zeros((M, nbp), dtype)
    Sp[:, :S.shape[1]] = S
    ph = np.zeros((M, nbp), dtype)
    if phase is not None:
        ph[:, :phase.shape[1]] = phase
    X = np.concatenate((Sp * np.cos(ph), Sp * np.sin(ph)), 1).astype(dtype)
    alpha = dtype(momentum / (1.0 + momentum))
    prev = np.zeros_like(X)
    for _ in range(n_iter):
        R = _frames(_ola(X @ inv.T, w, n, dtype), w, M) @ fwd.T
        a = R - alpha * prev
        prev = R
        are, aim = a[:, :nbp], a[:, nbp:]
        mag = np.sqrt(are * are + aim * aim)
        safe = np.where(mag > 0, mag, 1)
        X = np.concatenate((np.where(mag > 0, Sp * are / safe, Sp), np.where(mag > 0, Sp * aim / safe, 0)), 1).astype(dtype)
    return _ola(X @ inv.T, w, n, dtype)


def mel_of(wav):
    return mel_ref.melspectrogram(np.asarray(wav, dtype=np.float64))


# ---------------------------------------------------------------------------------------------- tests
def test_sparse_mel_table_rebuilds_the_dense_basis():
    tb = tables()
    W, bf, bw, rng = tb["mel_basis"], tb["bin_filt"], tb["bin_w"], tb["filt_range"]
    assert W.shape == (NM, tb["nbp"]) and bf.shape == bw.shape == (tb["nbp"], 2)
    dense = np.zeros_like(W)
    for j in range(W.shape[1]):
        for s in range(2):
            if bf[j, s] >= 0:
                dense[bf[j, s], j] += bw[j, s]
            else:
                assert bw[j, s] == 0.0
    assert np.array_equal(dense, W)
    assert ((bf >= 0).sum(1) <= 2).all() and ((bf >= 0).sum(1) == 2).any()
    for f in range(NM):                      # the bin range is exactly the filter's support
        lo, hi = rng[f]
        nz = np.nonzero(W[f])[0]
        assert (lo, hi) == (nz[0], nz[-1] + 1)
    assert not tb["ola_norm"]                 # the lws window at hop fsize/4 overlap-adds to 1
    assert abs(tb["step"] * np.linalg.norm(W, 2) ** 2 - 1.0) < 1e-12
    np.testing.assert_allclose(tb["pinv"], np.linalg.pinv(W), rtol=0, atol=1e-12)


def test_inverse_basis_inverts_the_forward_dft():
    from dvae_amd.frontend import dft_basis
    tb = tables()
    inv, fwd = tb["inv_basis"], dft_basis(FS, tb["nbp"])
    assert inv.shape == (FS, 2 * tb["nbp"])
    assert np.abs(inv @ fwd - np.eye(FS)).max() <= 1e-12
    x = np.random.RandomState(0).standard_normal((3, FS))
    np.testing.assert_allclose(inv @ (fwd @ x.T), x.T, rtol=0, atol=1e-12)
    # and it is irfft on the one-sided spectrum
    D = np.fft.rfft(x, axis=1)
    Xp = np.zeros((3, 2 * tb["nbp"]))
    Xp[:, :tb["nb"]], Xp[:, tb["nbp"]:tb["nbp"] + tb["nb"]] = D.real, D.imag
    np.testing.assert_allclose(Xp @ inv.T, np.fft.irfft(D, n=FS, axis=1), rtol=0, atol=1e-12)


def test_tables_match_the_frontend_constants():
    """MelFrontend and the inverse share one window and one mel basis"""
    from dvae_amd.frontend import lws_window, mel_basis
    tb = tables()
    np.testing.assert_array_equal(tb["window"], lws_window(FS, HOP))
    np.testing.assert_allclose(tb["window"], mel_ref.lws_window(), rtol=0, atol=1e-15)
    np.testing.assert_allclose(tb["mel_basis"][:, :tb["nb"]], mel_ref.mel_basis(), rtol=0, atol=1e-12)
    assert np.array_equal(mel_basis(mel_ref.SAMPLE_RATE, FS, NM, mel_ref.FMIN, mel_ref.FMAX, tb["nbp"]), tb["mel_basis"])


def test_restated_istft_of_the_stft_is_exact():
    """iSTFT o STFT on the lws framing (the operator pair the GPU gather implements) is the identity on length-n signals"""
    tb = tables()
    for n in (256, 4096, 32000):
        x = signal(n, 1).astype(np.float64)
        D = mel_ref.lws_stft(x)                      # [M, nb]
        M = D.shape[0]
        assert (M - 3) * HOP == n
        y = griffin_lim(np.abs(D), np.angle(D), 0, tb=tb)
        assert np.abs(y - x).max() <= 1e-12


def test_restated_round_trip_mel_to_wav_to_mel():
    """wav -> mel -> pinv + 200 projected-gradient steps -> 32 Griffin-Lim iterations -> mel, on three signals"""
    tb = tables()
    for seed in (1, 3, 5):
        mel = mel_of(signal(32000, seed))
        X = linear_magnitude(mel, 200, tb)
        assert X.min() >= 0.0 and np.median(residual(X, mel, tb)) < 1e-3
        ph = 2 * np.pi * np.random.RandomState(seed).random_sample((mel.shape[1], tb["nb"]))
        wav = griffin_lim(X, ph, 32, tb=tb)
        back = mel_of(wav)
        assert back.shape == mel.shape
        d = np.abs(back - mel)
        assert d.mean() <= 0.01, (seed, d.mean())
