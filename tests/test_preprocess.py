"""Corpus preprocessing (dvae_amd.preprocess), the CPU half: the resampy kaiser_best restatement in float64 numpy (also used by
tests/test_hip_preprocess.py and scripts/preprocess_bench.py) anchored to physics, the host filter tables, the wav reader and
the CLI's argument checks.

resampy.resample(x, sr_old, sr_new, filter="kaiser_best") (resampy/interp.py resample_f), restated: ratio = sr_new / sr_old,
scale = min(1, ratio), table win (x ratio when downsampling) and delta = its forward difference, index_step =
int(scale * 512); output t of int(n * ratio): x_t = t / ratio, m = int(x_t), frac = scale (x_t - m), left taps i < min(m + 1,
(nwin - off) // index_step) on x[m - i], right taps k < min(n - m - 1, (nwin - off') // index_step) on x[m + 1 + k] with
frac' = scale - frac; weight = win[off + j index_step] + eta delta[...], off = int(frac 512), eta = frac 512 - off."""
import os
import struct
import subprocess
import sys
import wave

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dvae_amd  # noqa: E402,F401
from dvae_amd.preprocess import (kaiser_best_window, read_wav, resample_filter, resample_lengths)  # noqa: E402

RATES = (48000, 44100, 32000, 24000, 22050, 8000)


def _taps(n, sr_old, sr_new, t):
    """per output t (int array): m, and (off, eta) of the left and right wings, by the float64 formula"""
    ratio = float(sr_new) / sr_old
    scale = min(1.0, ratio)
    x = t.astype(np.float64) / ratio
    m = x.astype(np.int64)
    frac = scale * (x - m)
    fl = frac * 512
    offl = fl.astype(np.int64)
    fr = (scale - frac) * 512
    offr = fr.astype(np.int64)
    return m, offl, fl - offl, offr, fr - offr


def resample_ref(x, sr_old, sr_new=16000, dtype=np.float64, fix=True):
    """the restatement above, vectorised over outputs, sequential over taps (left wing i = 0.., then right wing k = 0..,
    resampy's order).  dtype float32: weights rounded to fp32, products and sums in fp32 (the `f32seq` yardstick).
    fix: librosa's fix=True (zero-pad to ceil(n * ratio))."""
    x = np.asarray(x, dtype=np.float64)
    if sr_old == sr_new:
        return x.astype(dtype)
    n = x.shape[0]
    ratio = float(sr_new) / sr_old
    n_valid = int(n * ratio)
    if n_valid < 1:
        raise ValueError("too short")
    win, num_table, _ = kaiser_best_window()
    if ratio < 1:
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    nwin = win.shape[0]
    step = int(min(1.0, ratio) * num_table)
    t = np.arange(n_valid)
    m, offl, etal, offr, etar = _taps(n, sr_old, sr_new, t)
    xs = x.astype(dtype)
    y = np.zeros(n_valid, dtype=dtype)
    for (off, eta, cnt_fn, src) in ((offl, etal, lambda o: np.minimum(m + 1, (nwin - o) // step), lambda j: m - j),
                                    (offr, etar, lambda o: np.minimum(n - m - 1, (nwin - o) // step), lambda j: m + 1 + j)):
        cnt = cnt_fn(off)
        for j in range(int(cnt.max()) if cnt.size else 0):
            live = j < cnt
            idx = np.where(live, off + j * step, 0)
            w = (win[idx] + eta * delta[idx]).astype(dtype)
            v = xs[np.where(live, src(j), 0)]
            y = np.where(live, (y + w * v).astype(dtype), y)
    if fix:
        y = np.concatenate([y, np.zeros(resample_lengths(n, sr_old, sr_new)[1] - n_valid, dtype=dtype)])
    return y


def normalize_ref(wav, target_dbfs=-30.0, increase_only=True):
    """audio.py:121-127 in float64 -> (wav, gain | None)"""
    ms = float(np.mean(np.asarray(wav, dtype=np.float64) ** 2))
    if ms == 0.0:
        return wav, None
    change = target_dbfs - 10 * np.log10(ms)
    if change < 0 and increase_only:
        return wav, 1.0
    g = 10 ** (change / 20)
    return wav * g, g


def tone(n, sr, f, phase=0.3):
    return np.sin(2 * np.pi * f * np.arange(n) / sr + phase)


# ---------------------------------------------------------------------------------------------------------- filter table
def test_filter_table_construction():
    win, num_table, rolloff = kaiser_best_window()
    assert win.shape == (32769,) and num_table == 512
    assert win[0] == rolloff
    # sinc zeros at multiples of 512 / rolloff (approximately: the table is sampled every 1/512 of a zero crossing)
    for k in (1, 2, 5, 20):
        pos = k * 512 / rolloff
        i = int(round(pos))
        assert abs(win[i]) < 2e-3 * abs(win[0]), (k, win[i])
        assert np.sign(win[int(np.floor(pos)) - 2]) != np.sign(win[int(np.ceil(pos)) + 2])
    t = resample_filter(48000)
    assert (t["P"], t["Q"], t["index_step"]) == (1, 3, 170)          # int(512 / 3): truncated, not 170.67
    assert t["taps"] == 383 and np.count_nonzero(t["weights"][0]) == 383    # 192 left + 191 right
    assert resample_filter(44100)["index_step"] == int(160 / 441 * 512) == 185
    assert resample_filter(8000)["index_step"] == 512 and resample_filter(8000)["P"] == 2
    assert resample_filter(44100)["weights"].shape[0] == 160 and resample_filter(22050)["P"] == 320
    # downsampling scales the table by the ratio
    assert resample_filter(48000)["win"][0] == pytest.approx(rolloff / 3, rel=1e-15)


def test_output_length_rule():
    for n, sr in ((48000, 48000), (3, 48000), (2, 48000), (44101, 44100), (7, 22050), (5, 8000)):
        nv, no = resample_lengths(n, sr)
        assert nv == int(n * (16000 / sr))
        assert no == int(np.ceil(n * 16000 / sr))
    assert resample_lengths(2, 48000)[0] == 0                       # resampy raises: too short
    assert resample_lengths(44101, 44100) == (16000, 16001)
    y = resample_ref(np.random.RandomState(0).randn(44101), 44100)
    assert y.shape == (16001,) and y[-1] == 0.0                     # fix=True pads the ceil


@pytest.mark.parametrize("sr", RATES)
def test_phase_table_selects_the_float64_taps(sr):
    """the GPU's exact integer phases pick the same input sample m and table offsets as the float64 formula, and the
    per-phase weights equal the formula's weights, at every output of lengths up to 600 s"""
    n = 600 * sr + 17
    t = np.arange(resample_lengths(n, sr)[0], dtype=np.int64)
    f = resample_filter(sr)
    P, Q = f["P"], f["Q"]
    m, offl, etal, offr, etar = _taps(n, sr, 16000, t)
    assert np.array_equal(m, t * Q // P)
    ph = t * Q - m * P
    sn, sd = (P, Q) if sr > 16000 else (1, 1)
    assert np.array_equal(offl, (512 * sn * ph) // (sd * P))
    assert np.array_equal(offr, (512 * sn * (P - ph)) // (sd * P))
    # weights of the phase table against the formula at a few hundred outputs: the formula's eta carries the rounding of
    # t / ratio (~1e-9 of a table step at 600 s), the table's is exact
    win, delta, step, base = f["win"], f["delta"], f["index_step"], f["base"]
    for tt in np.linspace(0, len(t) - 1, 200).astype(np.int64):
        p = int(ph[tt])
        i = np.arange((win.shape[0] - offl[tt]) // step)
        wl = win[offl[tt] + i * step] + etal[tt] * delta[offl[tt] + i * step]
        assert np.allclose(f["weights"][p, base - i], wl, rtol=0, atol=1e-9)
        k = np.arange((win.shape[0] - offr[tt]) // step)
        wr = win[offr[tt] + k * step] + etar[tt] * delta[offr[tt] + k * step]
        assert np.allclose(f["weights"][p, base + 1 + k], wr, rtol=0, atol=1e-9)


# ---------------------------------------------------------------------------------------------- the restatement, physics
def _dc_gain(sr):
    """the filter's gain at 0 Hz, measured: the interior of a resampled constant.  Not 1 when downsampling: resampy
    truncates index_step (int(512 / 3) = 170 at 48 kHz), so its wings sample the sinc 512 scale / index_step times too
    densely (+0.39 % at 48 kHz, less the taper's share) -- part of the contract, kept"""
    y = resample_ref(np.ones(sr), sr)
    g = y[4000:12000]
    assert np.ptp(g) < 1e-4                                          # phase-dependent at 44.1 kHz (7e-5)
    return float(g.mean())


@pytest.mark.parametrize("sr", (48000, 44100))
def test_1khz_tone_is_the_analytic_16k_tone(sr):
    g = _dc_gain(sr)
    step = int(512 * 16000 / sr)
    assert 1.0 < g < 512 * 16000 / sr / step                        # between 1 and the sampling-density bound
    y = resample_ref(tone(sr, sr, 1000.0), sr)
    want = g * tone(16000, 16000, 1000.0)
    interior = slice(800, 16000 - 800)
    assert np.max(np.abs(y[interior] - want[interior])) < 1e-3


def _suppression_db(sr, f=12000.0):
    y = resample_ref(tone(sr, sr, f), sr)[800:16000 - 800]
    return 20 * np.log10(np.sqrt(np.mean(y ** 2)) / np.sqrt(0.5))


def test_12khz_tone_above_the_new_nyquist_is_suppressed():
    """Kaiser beta = 14.77 puts the stopband ~140 dB down, and that is what 32 kHz -> 16 kHz (index_step = 256, exact)
    shows.  Where resampy truncates index_step (48 kHz: 170 for 170.67) the right wing's table offset keeps the fraction
    that the step drops, the two wings no longer sample one filter, and the 12 kHz tone (aliasing to 4 kHz) is only ~72 dB
    down.  The contract keeps the truncation, so 80 dB is not reachable at 48 kHz: the bound there is 70 dB."""
    assert _suppression_db(32000) <= -140.0
    assert _suppression_db(48000) <= -70.0
    assert _suppression_db(44100) <= -70.0


def test_8k_to_16k_keeps_a_1khz_tone():
    assert abs(_dc_gain(8000) - 1.0) < 1e-6                          # upsampling: index_step = 512 exactly
    y = resample_ref(tone(8000, 8000, 1000.0), 8000)
    want = tone(16000, 16000, 1000.0)
    interior = slice(800, 16000 - 800)
    assert np.max(np.abs(y[interior] - want[interior])) < 1e-3


def test_f32seq_is_close_to_f64():
    x = np.random.RandomState(1).uniform(-1, 1, 4801)
    a, b = resample_ref(x, 48000), resample_ref(x, 48000, dtype=np.float32)
    d = np.max(np.abs(a - b))
    assert 0 < d < 1e-5


def test_normalize_ref():
    w = 0.01 * np.ones(100)
    out, g = normalize_ref(w)
    assert g == pytest.approx(10 ** ((-30 + 40) / 20)) and np.allclose(10 * np.log10(np.mean(out ** 2)), -30)
    loud, g = normalize_ref(0.5 * np.ones(10))
    assert g == 1.0 and loud[0] == 0.5
    assert normalize_ref(np.zeros(10))[1] is None


# ----------------------------------------------------------------------------------------------------------- read_wav
def _stdlib_wav(path, x_int16, sr, ch=1):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(ch)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.asarray(x_int16, dtype="<i2").tobytes())


def _riff(path, tag, ch, sr, bits, data, extensible=False, extra_chunks=b""):
    align = ch * bits // 8
    if extensible:
        guid = struct.pack("<H", tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, ch, sr, sr * align, align, bits, 22, bits, 0) + guid
    else:
        fmt = struct.pack("<HHIIHH", tag, ch, sr, sr * align, align, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + extra_chunks
    body += b"data" + struct.pack("<I", len(data)) + data + (b"\x00" if len(data) & 1 else b"")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def test_read_wav_pcm16_stdlib(tmp_path):
    x = np.array([0, 1, -1, 32767, -32768, 1234], dtype=np.int16)
    _stdlib_wav(tmp_path / "a.wav", x, 48000)
    w, sr = read_wav(tmp_path / "a.wav")
    assert sr == 48000 and w.dtype == np.float32
    assert np.array_equal(w, (x / 32768.0).astype(np.float32))


def test_read_wav_float32_s24_extensible_stereo_list(tmp_path):
    f = np.array([0.5, -0.25, 1.5, 1e-8], dtype="<f4")
    _riff(tmp_path / "f.wav", 3, 1, 22050, 32, f.tobytes())
    w, sr = read_wav(tmp_path / "f.wav")
    assert sr == 22050 and np.array_equal(w, f)
    s24 = np.array([0, 1, -1, 2 ** 23 - 1, -2 ** 23, 4660], dtype=np.int64)
    raw = b"".join(int(v & 0xFFFFFF).to_bytes(3, "little") for v in s24)
    _riff(tmp_path / "s24.wav", 1, 1, 44100, 24, raw)           # 18 bytes of data: even; add one odd chunk below
    w, sr = read_wav(tmp_path / "s24.wav")
    assert sr == 44100 and np.array_equal(w, (s24 / 2.0 ** 23).astype(np.float32))
    d = np.array([3, -7, 32000, -2], dtype="<i2")
    _riff(tmp_path / "ext.wav", 1, 1, 16000, 16, d.tobytes(), extensible=True)
    assert np.array_equal(read_wav(tmp_path / "ext.wav")[0], (d / 32768.0).astype(np.float32))
    fx = np.array([0.125, -0.5], dtype="<f8")
    _riff(tmp_path / "ext64.wav", 3, 1, 16000, 64, fx.tobytes(), extensible=True)
    assert np.array_equal(read_wav(tmp_path / "ext64.wav")[0], fx.astype(np.float32))
    st = np.array([[100, 300], [-5, 7], [32767, 32767]], dtype="<i2")
    lst = b"LIST" + struct.pack("<I", 5) + b"INFOx" + b"\x00"       # odd-size chunk + pad byte
    _riff(tmp_path / "st.wav", 1, 2, 8000, 16, st.tobytes(), extra_chunks=lst)
    w, sr = read_wav(tmp_path / "st.wav")
    want = (st / 32768.0).astype(np.float32).mean(axis=1, dtype=np.float32)
    assert sr == 8000 and np.array_equal(w, want)
    u8 = np.array([128, 0, 255, 64], dtype=np.uint8)
    _riff(tmp_path / "u8.wav", 1, 1, 8000, 8, u8.tobytes())
    assert np.array_equal(read_wav(tmp_path / "u8.wav")[0], ((u8.astype(np.float32) - 128) / 128).astype(np.float32))
    s32 = np.array([2 ** 31 - 1, -2 ** 31, 12345678], dtype="<i4")
    _riff(tmp_path / "s32.wav", 1, 1, 8000, 32, s32.tobytes())
    assert np.array_equal(read_wav(tmp_path / "s32.wav")[0], (s32 / 2.0 ** 31).astype(np.float32))


def test_read_wav_duration_cap(tmp_path):
    x = (np.arange(3000) % 200 - 100).astype(np.int16)
    _stdlib_wav(tmp_path / "c.wav", x, 8)                        # 375 s at 8 Hz ...
    assert read_wav(tmp_path / "c.wav")[0].shape == (3000,)
    _stdlib_wav(tmp_path / "d.wav", np.zeros(5000, dtype=np.int16), 8)   # ... 625 s: cut to 600 s = 4800 frames
    assert read_wav(tmp_path / "d.wav")[0].shape == (4800,)
    assert read_wav(tmp_path / "d.wav", duration=1.0)[0].shape == (8,)


def test_read_wav_rejects_with_the_path(tmp_path):
    _riff(tmp_path / "alaw.wav", 6, 1, 8000, 8, b"\x01\x02")
    with pytest.raises(ValueError, match="alaw.wav"):
        read_wav(tmp_path / "alaw.wav")
    (tmp_path / "x.flac").write_bytes(b"fLaC\x00\x00\x00\x22" + bytes(40))
    with pytest.raises(ValueError, match="x.flac"):
        read_wav(tmp_path / "x.flac")
    _stdlib_wav(tmp_path / "t.wav", np.arange(100, dtype=np.int16), 16000)
    raw = (tmp_path / "t.wav").read_bytes()
    (tmp_path / "t.wav").write_bytes(raw[:-50])
    with pytest.raises(ValueError, match="t.wav.*truncated"):
        read_wav(tmp_path / "t.wav")


# --------------------------------------------------------------------------------------------------------- CLI checks
def _cli(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "dvae_amd.preprocess"] + args, env=env, capture_output=True, text=True,
                          timeout=300)


def test_cli_requires_no_trim_and_a_known_dataset(tmp_path):
    root = tmp_path / "data"
    (root / "VCTK-Corpus" / "wav16" / "p1").mkdir(parents=True)
    out = tmp_path / "out"
    r = _cli([str(root), "-o", str(out)])
    assert r.returncode != 0 and "--no_trim" in r.stderr and "webrtcvad" in r.stderr
    assert not out.exists() and not (root / "SV2TTS").exists()
    r = _cli([str(root), "-o", str(out), "-d", "librispeech_other", "--no_trim"])
    assert r.returncode != 0 and "VCTK" in r.stderr and "librispeech_other" in r.stderr
    assert not out.exists()
