"""Silence trimming (dvae_amd.preprocess --trim), the CPU half: the integer restatement of tests/vad_ref.py against the
reference's floating-point smoothing formula, the percentile / threshold rule on hand-built bins, a synthetic utterance
whose kept windows follow from its burst borders, the constants the package and the header share with it, the CLI's flag
checks, and the host pipeline of tests/test_preprocess_pipeline.py with trim=True."""
import itertools
import os
import re
import subprocess
import sys
import wave

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dvae_amd  # noqa: E402,F401
import vad_ref as V  # noqa: E402
from dvae_amd import preprocess  # noqa: E402


# ---------------------------------------------------------------------------------------------------------- constants
def test_constants_agree_between_package_header_and_reference():
    from dvae_amd import _lib
    assert (preprocess.VAD_WINDOW, preprocess.VAD_MA_WIDTH, preprocess.VAD_MAX_SILENCE, preprocess.VAD_PREEMPH) == \
        (V.WINDOW, V.MA_WIDTH, V.MAX_SILENCE, V.PREEMPH) == (480, 8, 6, 0.97)
    assert (preprocess.VAD_BINS, preprocess.VAD_BIN_OFFSET, preprocess.VAD_BIN_FLOOR, preprocess.VAD_BIN_ABOVE_P10,
            preprocess.VAD_BIN_BELOW_P90) == (V.BINS, V.BIN_OFFSET, V.BIN_FLOOR, V.ABOVE_P10, V.BELOW_P90) == (96, 80, 66, 3, 5)
    assert (preprocess.TOO_SHORT_TO_TRIM, preprocess.NO_SPEECH) == (V.TOO_SHORT, V.NO_SPEECH)
    hdr = open(os.path.join(ROOT, "include", "dvae_hip.h")).read()
    defs = dict(re.findall(r"^#define (DVAE_VAD_[A-Z0-9_]+) (\S+)$", hdr, flags=re.M))
    assert defs == {"DVAE_VAD_WINDOW": "480", "DVAE_VAD_MA_WIDTH": "8", "DVAE_VAD_MAX_SILENCE": "6", "DVAE_VAD_PREEMPH": "0.97",
                    "DVAE_VAD_BINS": "96", "DVAE_VAD_BIN_OFFSET": "80", "DVAE_VAD_BIN_FLOOR": "66",
                    "DVAE_VAD_BIN_ABOVE_P10": "3", "DVAE_VAD_BIN_BELOW_P90": "5"}
    assert "dvae_vad_trim" in _lib.SIGNATURES and len(_lib.SIGNATURES["dvae_vad_trim"][1]) == 16
    assert re.search(r"#define DVAE_ABI_VERSION (\d+)", hdr).group(1) == str(_lib.ABI_VERSION)


# ---------------------------------------------------------------------------------------------------------- smoothing
def test_integer_smoothing_is_the_cumsum_round_dilation_formula():
    pytest.importorskip("scipy.ndimage")
    n = 0
    for W in range(0, 13):
        for bits in itertools.product((0, 1), repeat=W):
            mi, ki = V.smooth(bits)
            mf, kf = V.smooth_by_formula(bits)
            assert np.array_equal(mi, mf) and np.array_equal(ki, kf), bits
            n += 1
    assert n == 2 ** 13 - 1
    rs = np.random.RandomState(0)
    for i in range(200):
        W = int(rs.randint(13, 400))
        flags = (rs.rand(W) < rs.uniform(0.05, 0.95)).astype(np.int64)
        if i % 3 == 0:                                   # long runs and gaps, as a detector produces them
            flags = np.repeat(flags[:W // 5 + 1], 5)[:W]
        mi, ki = V.smooth(flags)
        mf, kf = V.smooth_by_formula(flags)
        assert np.array_equal(mi, mf) and np.array_equal(ki, kf), (i, W)


def test_smoothing_by_hand():
    ones = lambda W: np.ones(W, np.int64)
    assert V.smooth(ones(4))[1].sum() == 0               # 4 flags never make 5 of 8
    assert V.smooth(ones(5))[0].tolist() == [1, 1, 1, 1, 0] and V.smooth(ones(5))[1].tolist() == [1] * 5
    m, k = V.smooth(ones(9))
    assert m.tolist() == [1] * 8 + [0] and k.all()
    # a run of flags [a, b) (long enough) is masked over [a, b - 1) and kept over [a - 3, b + 2)
    f = np.zeros(40, np.int64)
    f[10:20] = 1
    m, k = V.smooth(f)
    assert np.nonzero(m)[0].tolist() == list(range(10, 19)) and np.nonzero(k)[0].tolist() == list(range(7, 22))
    # masked runs 6 windows apart are bridged, 7 apart leave one window out
    for gap, dropped in ((6, 0), (7, 1), (9, 3)):
        f = np.zeros(60, np.int64)
        f[5:15] = 1                                       # masked [5, 14)
        f[13 + gap + 1:13 + gap + 11] = 1                 # masked from 14 + gap on
        m, k = V.smooth(f)
        assert m[14:14 + gap].sum() == 0 and m[13] == 1 and m[14 + gap] == 1
        assert (k[14:14 + gap] == 0).sum() == dropped, (gap, k)


# ----------------------------------------------------------------------------------------------- percentiles, threshold
def _brute_threshold(b):
    s = np.sort(np.asarray(b))
    W = len(s)
    b10, b90 = int(s[-(-W // 10) - 1]), int(s[-(-9 * W // 10) - 1])
    return b10, b90, max(66, min(b10 + 3, b90 - 5))


def test_threshold_rule_on_hand_built_bins():
    assert V.threshold([70]) == (70, 70, 66)                          # W = 1: b90 - 5 = 65 under the floor
    assert V.threshold([80]) == (80, 80, 75)
    nine = [60] * 1 + [70] * 7 + [90]
    assert V.threshold(nine) == (60, 90, 66)                          # W = 9: ceil(0.9) = 1st, ceil(8.1) = 9th; 63 -> floor 66
    ten = [65] + [70] * 8 + [90]
    assert V.threshold(ten) == (65, 70, 66)                           # W = 10: 1st and 9th; min(68, 65) = 65 -> 66
    eleven = [65] + [64] + [80] * 9
    assert V.threshold(eleven) == (65, 80, 68)                        # W = 11: ceil(1.1) = 2nd, ceil(9.9) = 10th; b10 + 3
    assert V.threshold([72] * 50) == (72, 72, 67)                     # all bins equal: b90 - 5, everything flagged
    assert V.threshold([50] * 30) == (50, 50, 66)                     # the floor clamp: nothing flagged
    assert V.threshold([69] * 50 + [76] * 50) == (69, 76, 71)         # b90 - 5 under b10 + 3
    assert V.threshold([60] * 50 + [90] * 50) == (60, 90, 66)
    assert V.threshold([68] * 50 + [90] * 50) == (68, 90, 71)         # b10 + 3 under b90 - 5
    assert V.threshold([]) == (0, 0, 66)
    rs = np.random.RandomState(1)
    for W in list(range(1, 40)) + [99, 100, 101, 1000]:
        b = rs.randint(0, 96, W)
        assert V.threshold(b) == _brute_threshold(b), W


def test_bins_come_from_the_exponent_field():
    E = np.array([0.0, 5e-324, 2.0 ** -1022 * 0.99, 2.0 ** -81, 2.0 ** -80, 1.99 * 2.0 ** -80, 2.0 ** -14, 1.0, 1.5, 2.0,
                  2.0 ** 15, 2.0 ** 16 * 0.999, 2.0 ** 300, np.inf])
    assert V.bins_of(E).tolist() == [0, 0, 0, 0, 0, 0, 66, 80, 80, 81, 95, 95, 95, 95]
    d = V.pow2_distance(np.array([1.0, 1.0 + 1e-12, 2.0 - 1e-12, 1.5, 0.0, 3e-5]))
    assert d[0] == 0 and d[1] < 2e-12 and d[2] < 2e-12 and d[3] == 0.5 and np.isinf(d[4]) and d[5] > 0.01


def test_energy_carries_the_predecessor_across_windows():
    y = np.zeros(3 * 480 + 100)
    y[0], y[479], y[480], y[1439], y[1440] = 1.0, 2.0, 0.0, 4.0, 100.0
    E = V.energies(y)
    assert E.shape == (3,)
    assert E[0] == pytest.approx(1.0 + 0.97 ** 2 + 4.0)              # y[0] - 0, y[1] - 0.97 y[0], y[479]
    assert E[1] == pytest.approx((0.97 * 2.0) ** 2)                   # the first sample of window 1 sees y[479]
    assert E[2] == pytest.approx(16.0)                                # the tail behind 3 windows is dropped
    assert V.energies(np.ones(479)).shape == (0,) and V.skip_reason(np.ones(479)) == V.TOO_SHORT
    assert V.skip_reason(np.zeros(4800)) == V.NO_SPEECH and V.skip_reason(1e-5 * np.ones(4800)) == V.NO_SPEECH


# -------------------------------------------------------------------------------------------------- synthetic utterance
@pytest.mark.parametrize("seed", range(5))
def test_synthetic_utterance_keeps_what_its_burst_borders_predict(seed):
    rs = np.random.RandomState(seed)
    W = 200
    y = V.floor_noise(rs, W * 480 + 77)
    # three bursts with borders inside windows, at least 100 samples from a window's edge
    edges = [(22 * 480 + 130, 61 * 480 + 250), (66 * 480 + 300, 109 * 480 + 120), (150 * 480 + 200, 171 * 480 + 350)]
    pred = np.zeros(W, np.int64)
    for a, b in edges:
        y[a:b] += V.burst(rs, b - a)
        pred[a // 480:b // 480 + 1] = 1                                # every window the burst reaches into
    r = V.detect(y.astype(np.float32))
    assert r["W"] == W and (r["b10"], r["b90"], r["t"]) == (69, 76, 71), (r["b10"], r["b90"], r["t"])
    for a, b in edges:
        full = slice(-(-a // 480), b // 480)
        assert r["flags"][full].all()                                  # every fully covered window
    assert np.array_equal(r["flags"], pred)
    want = V.smooth(pred)[1]
    # flags [a, b) are masked over [a, b - 1) and kept over [a - 3, b + 2): [19, 64), [63, 112) and [147, 174)
    assert np.array_equal(r["keep"], want) and r["K"] == int(want.sum()) == 93 + 27
    assert not r["keep"][:19].any() and r["keep"][19:112].all()        # the 4 unflagged windows 62 .. 65 stay: a short pause
    assert not r["keep"][112:147].any() and r["keep"][147:174].all() and not r["keep"][174:].any()
    out = V.trim(y.astype(np.float32), r)
    assert out.shape == (480 * 120,) and out.dtype == np.float32
    assert np.array_equal(out[:480], y.astype(np.float32)[19 * 480:20 * 480])
    assert np.array_equal(out[-480:], y.astype(np.float32)[173 * 480:174 * 480])
    assert np.array_equal(r["dst"][r["keep"] == 1], np.arange(120))


def test_all_floor_is_kept_and_deep_silence_is_not():
    rs = np.random.RandomState(7)
    r = V.detect(V.floor_noise(rs, 50 * 480).astype(np.float32))
    assert r["t"] == 66 and r["K"] == 50                               # b90 - 5 under every bin: nearly-all-speech rule
    r = V.detect(V.floor_noise(rs, 50 * 480, dbfs=-95.0).astype(np.float32))
    assert r["t"] == 66 and r["K"] == 0 and V.skip_reason(None, r) == V.NO_SPEECH


# ------------------------------------------------------------------------------------------------------------------ CLI
def _cli(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "dvae_amd.preprocess"] + args, env=env, capture_output=True, text=True,
                          timeout=300)


def test_cli_trim_and_no_trim_exclude_each_other(tmp_path):
    root = tmp_path / "data"
    (root / "VCTK-Corpus" / "wav16" / "p1").mkdir(parents=True)
    out = tmp_path / "out"
    r = _cli([str(root), "-o", str(out), "--trim", "--no_trim"])
    assert r.returncode == 2 and "--trim" in r.stderr and "--no_trim" in r.stderr and "exclude" in r.stderr
    assert not out.exists() and not (root / "SV2TTS").exists()
    r = _cli([str(root), "-o", str(out)])                              # neither: the message of before, and a pointer
    assert r.returncode == 2 and preprocess.NO_TRIM_MESSAGE in r.stderr and "--trim" in r.stderr.splitlines()[-1]
    assert not out.exists()
    assert preprocess.NO_TRIM_MESSAGE.startswith("Package 'webrtcvad' not found.") and \
        preprocess.NO_TRIM_MESSAGE.endswith("use --no_trim to disable this error message.")
    # an empty tree with --trim: nothing to do, no GPU touched, the summary says what was trimmed only when trimming ran
    r = _cli([str(root), "-o", str(out), "--trim"])
    assert r.returncode == 0 and r.stdout.strip() == "preprocess: 0 written, 0 already present, 0 skipped", (r.stdout, r.stderr)


def _tree(root, n_spk=2, n_utt=7, sr=16000, seconds=0.5):
    base = root / "VCTK-Corpus" / "wav16"
    for s in range(n_spk):
        d = base / f"p{225 + s}"
        d.mkdir(parents=True)
        for u in range(n_utt):
            v = ((np.arange(int(sr * seconds)) * (s + u + 1)) % 2000 - 1000).astype("<i2")
            with wave.open(str(d / f"p{225 + s}_{u:03d}.wav"), "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(sr)
                w.writeframes(v.tobytes())
    return base


def test_pipeline_with_a_stub_batch_and_trim(tmp_path):
    """tests/test_preprocess_pipeline.py's check with trim=True: outputs and `_sources.txt` lines are those of the plain
    order whatever the batch size, worker count and window; the injected run_batch keeps its (wavs, srs) signature, its
    skips reach the summary, and its trim_stats the totals."""
    base = _tree(tmp_path)
    counts = dict(total=0, kept=0)

    def run_batch(wavs, srs):
        assert all(sr == 16000 for sr in srs)
        out = []
        for w in wavs:
            r = V.detect(w)
            if r["K"] == 0:
                out.append((None, V.skip_reason(w, r)))
                continue
            counts["total"] += w.shape[0]
            counts["kept"] += 480 * r["K"]
            out.append((np.full((80, r["K"]), float(w.shape[0] % 7), dtype=np.float32), None))
        return out

    run_batch.trim_stats = counts
    short = base / "p225" / "p225_short.wav"
    with wave.open(str(short), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.full(400, 1000, "<i2").tobytes())
    Ks = {p.name: V.detect(preprocess.read_wav(p)[0])["K"] for p in sorted(base.rglob("*.wav")) if p != short}
    kept = 480 * sum(Ks.values())
    assert len(Ks) == 14 and min(Ks.values()) >= 5 and 0 < kept < 14 * 8000
    snaps = []
    for i, (bs, wk, ahead) in enumerate(((0.4, 1, 1), (3.0, 16, None), (100.0, 3, 2))):
        counts.update(total=0, kept=0)
        out = tmp_path / f"o{i}"
        out.mkdir()
        st = preprocess.preprocess_vctk(base, out, batch_seconds=bs, workers=wk, run_batch=run_batch, decode_ahead=ahead,
                                        trim=True)
        assert st["written"] == 14 and st["skipped"] == [(str(short), V.TOO_SHORT)]
        assert st["total_samples"] == 14 * 8000 and st["trimmed_samples"] == 14 * 8000 - kept
        snaps.append({str(p.relative_to(out)): p.read_bytes() for p in sorted(out.rglob("*")) if p.is_file()})
    assert snaps[0] == snaps[1] == snaps[2]
    lines = snaps[0]["p225/_sources.txt"].decode().splitlines()
    assert [l.split(",")[0] for l in lines] == [f"p225_{u:03d}_mel.npy" for u in range(7)]
    assert np.load(tmp_path / "o0" / "p226" / "p226_003_mel.npy").shape == (80, Ks["p226_003.wav"])
    # without trim_stats (today's runners) the totals are absent, and trim=False is the default
    plain = lambda wavs, srs: [(np.zeros((80, 4), np.float32), None) for _ in wavs]
    out = tmp_path / "plain"
    out.mkdir()
    st = preprocess.preprocess_vctk(base, out, run_batch=plain)
    assert st["written"] == 15 and "trimmed_samples" not in st
