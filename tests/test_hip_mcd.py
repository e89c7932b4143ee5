"""Mel-cepstral distortion on the GPU (dvae_amd.evaluate): the DTW kernel, the feature pass and the voicing
flags against the float64 restatements of tests/test_mcd.py, batch independence and determinism, MCD end to end, and the
CLI on synthetic PCM-16 files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dvae_amd  # noqa: E402,F401
from dvae_amd import evaluate as ev  # noqa: E402
from test_mcd import dtw_ref, features_ref, harmonic, write_pcm16  # noqa: E402


@pytest.fixture(scope="module")
def fe():
    return ev.MelCepstrum()


def _seq(rs, n):
    return rs.randn(n, ev.DIM).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------- DTW
def test_dtw_matches_the_float64_restatement():
    rs = np.random.RandomState(10)
    shapes = [(1, 1), (1, 300), (300, 1), (37, 300), (300, 37), (1500, 1200), (4500, 4096)]
    xs = [_seq(rs, n) for n, _ in shapes]
    ys = [_seq(rs, m) for _, m in shapes]
    cost, length = ev.dtw_batch(xs, ys)
    assert cost.dtype == np.float64 and length.shape == (len(shapes),)
    for p, (x, y) in enumerate(zip(xs, ys)):
        c, l = dtw_ref(x, y)
        tol = 1e-4 if min(shapes[p]) >= 4096 else 1e-5
        assert abs(cost[p] - c) <= tol * c, (shapes[p], cost[p], c)
        assert length[p] == l, (shapes[p], length[p], l)


def test_dtw_empty_and_oversize():
    import torch
    from dvae_amd._lib import lib
    rs = np.random.RandomState(11)
    cost, length = ev.dtw_batch([np.zeros((0, ev.DIM), np.float32), _seq(rs, 5)], [_seq(rs, 9), _seq(rs, 5)])
    assert np.isnan(cost[0]) and length[0] == 0 and np.isfinite(cost[1]) and length[1] >= 5
    big = _seq(rs, ev.DTW_MAX_SHORT + 1)
    with pytest.raises(ValueError, match="DTW kernel supports"):
        ev.dtw_batch([big], [big])
    # the C entry point refuses it before launching, from its host copy of the table
    x = torch.zeros((ev.DTW_MAX_SHORT + 1, ev.DIM), device="cuda")
    pairs = np.array([[0, ev.DTW_MAX_SHORT + 1, 0, ev.DTW_MAX_SHORT + 1]], dtype=np.int64)
    pd = torch.from_numpy(pairs).cuda()
    out_c = torch.full((1,), 7.0, device="cuda", dtype=torch.float64)
    out_l = torch.full((1,), 7, device="cuda", dtype=torch.int64)
    rc = lib().dvae_dtw_batch(x.data_ptr(), x.data_ptr(), pd.data_ptr(), pairs.ctypes.data, 1, out_c.data_ptr(),
                              out_l.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and out_c.item() == 7.0 and out_l.item() == 7


def test_dtw_batch_independence_and_determinism():
    rs = np.random.RandomState(12)
    xs = [_seq(rs, int(n)) for n in rs.randint(1, 400, 64)]
    ys = [_seq(rs, int(n)) for n in rs.randint(1, 400, 64)]
    c1, l1 = ev.dtw_batch(xs, ys)
    c2, l2 = ev.dtw_batch(xs, ys)
    assert np.array_equal(c1.view(np.int64), c2.view(np.int64)) and np.array_equal(l1, l2)
    for p in range(64):
        c, l = ev.dtw_batch([xs[p]], [ys[p]])
        assert c.view(np.int64)[0] == c1.view(np.int64)[p] and l[0] == l1[p], p


# -------------------------------------------------------------------------------------------------------- features
def _signals():
    rs = np.random.RandomState(13)
    t = np.arange(24000) / 16000.0
    chirp = (0.4 * np.sin(2 * np.pi * (100 * t + 150 * t ** 2)) + 0.01 * rs.randn(t.size)).astype(np.float32)
    return [harmonic(16000, 120.0, seed=1), harmonic(12345, 233.0, seed=2, snr_db=20.0), chirp,
            (0.1 * rs.randn(8000)).astype(np.float32), harmonic(333, 400.0, seed=3)]


def test_features_match_the_float64_restatement(fe):
    sigs = _signals()
    got = fe.batch(sigs)
    for x, (mc, voiced) in zip(sigs, got):
        ref = features_ref(x)
        assert mc.shape == (ev.frame_count(len(x)), ev.DIM) and voiced.shape == (mc.shape[0],)
        loud = ref["r0"] >= ev.VOICED_REL_POWER * ref["r0"].max()
        err = np.max(np.abs(mc[loud] - ref["mc"][loud, :ev.DIM]))
        assert err <= 1e-4, (len(x), err)


def test_features_batch_independence(fe):
    import torch
    sigs = _signals()
    out = fe.packed(sigs)
    torch.cuda.synchronize()
    feats = out["feats"].cpu().numpy()
    mc = out["mc"].cpu().numpy()
    for s, x in enumerate(sigs):
        one = fe.packed([x])
        r0, M = out["table"][s, :2]
        k = out["count"][s]
        assert one["count"][0] == k
        assert np.array_equal(one["mc"].cpu().numpy(), mc[r0:r0 + M])
        assert np.array_equal(one["feats"].cpu().numpy()[:k], feats[r0:r0 + k])


# --------------------------------------------------------------------------------------------------------- voicing
def test_voicing_tone_noise_silence(fe):
    rs = np.random.RandomState(14)
    tone, noise, silence = harmonic(32000, 120.0, seed=4), (0.1 * rs.randn(32000)).astype(np.float32), \
        np.zeros(16000, np.float32)
    (_, v_tone), (_, v_noise), (_, v_sil) = fe.batch([tone, noise, silence])
    assert v_tone[4:-4].mean() >= 0.95, v_tone.mean()
    assert v_noise.mean() <= 0.05, v_noise.mean()
    assert not v_sil.any()


def test_voicing_flags_match_the_restatement(fe):
    import torch
    rs = np.random.RandomState(15)
    mixed = np.concatenate([harmonic(8000, 150.0, seed=5), 0.05 * rs.randn(6000), np.zeros(3000),
                            harmonic(9000, 600.0, seed=6, snr_db=10.0), 0.002 * harmonic(5000, 90.0, seed=7),
                            harmonic(7000, 75.0, seed=8, snr_db=5.0)]).astype(np.float32)
    out = fe.packed([mixed])
    torch.cuda.synchronize()
    v = out["voiced"].cpu().numpy().astype(bool)
    peak = out["peak"].cpu().numpy()
    ref = features_ref(mixed)
    near = (np.abs(ref["peak"] - ev.VOICED_PEAK) < 1e-3) | \
           (np.abs(ref["r0"] / ref["r0"].max() - ev.VOICED_REL_POWER) < 1e-3 * ev.VOICED_REL_POWER)
    bad = np.nonzero((v != ref["voiced"]) & ~near)[0]
    assert bad.size == 0, (bad[:10], peak[bad[:10]], ref["peak"][bad[:10]])
    assert 0.2 < v.mean() < 0.9, v.mean()
    assert np.max(np.abs(peak - ref["peak"])[ref["r0"] > 1e-6 * ref["r0"].max()]) < 1e-3
    assert out["count"][0] == v.sum()


# ------------------------------------------------------------------------------------------------------------- MCD
def _pair_signals():
    rs = np.random.RandomState(16)
    a = [harmonic(20000, 120.0, seed=20), harmonic(16000, 200.0, seed=21), harmonic(24000, 95.0, seed=22)]
    b = [harmonic(22000, 130.0, seed=23, harmonics=5), (harmonic(16000, 210.0, seed=24) + 0.05 * rs.randn(16000))
         .astype(np.float32), harmonic(19000, 300.0, seed=25, snr_db=15.0)]
    return a, b


def test_mcd_identical_and_swapped(fe):
    a, b = _pair_signals()
    same = ev.mcd_batch(a, a, features=fe)
    assert np.all(same["mcd"] == 0.0), same["mcd"]
    fwd = ev.mcd_batch(a, b, features=fe)
    rev = ev.mcd_batch(b, a, features=fe)
    assert np.all(np.isfinite(fwd["mcd"])) and np.all(fwd["mcd"] > 0)
    assert np.all(np.abs(fwd["mcd"] - rev["mcd"]) <= 1e-5 * fwd["mcd"]), (fwd["mcd"], rev["mcd"])
    assert np.array_equal(fwd["voiced_converted"], rev["voiced_reference"])


def test_mcd_matches_the_float64_pipeline(fe):
    a, b = _pair_signals()
    res = ev.mcd_batch(a, b, features=fe)
    flags = [v for _, v in fe.batch(a + b)]
    for p in range(len(a)):
        fx, fy = features_ref(a[p])["mc"][:, :ev.DIM], features_ref(b[p])["mc"][:, :ev.DIM]
        vx, vy = flags[p], flags[len(a) + p]
        assert res["voiced_converted"][p] == vx.sum() and res["voiced_reference"][p] == vy.sum()
        c, l = dtw_ref(fx[vx], fy[vy])
        ref = float(ev.mcd_from([c], [l])[0])
        assert abs(res["mcd"][p] - ref) <= 1e-3, (p, res["mcd"][p], ref)
    assert np.isclose(res["mean_mcd"], res["mcd"].mean(), rtol=1e-15)


def test_mcd_without_voiced_frames_is_nan(fe):
    a, _ = _pair_signals()
    res = ev.mcd_batch([a[0], np.zeros(8000, np.float32)], [np.zeros(4000, np.float32), a[1]], features=fe)
    assert np.all(np.isnan(res["mcd"])) and np.isnan(res["mean_mcd"])
    assert res["voiced_reference"][0] == 0 and res["voiced_converted"][1] == 0


# ------------------------------------------------------------------------------------------------------------- CLI
def _run(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "dvae_amd.evaluate"] + [str(a) for a in args], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=timeout)


def test_cli_end_to_end(tmp_path, fe):
    from dvae_amd.preprocess import read_wav, resample_batch
    a, b = _pair_signals()
    cdir, rdir = tmp_path / "p225_to_p226", tmp_path / "p226"
    cdir.mkdir()
    rdir.mkdir()
    write_pcm16(cdir / "convert_p225_to_p226_001.wav", a[0])
    write_pcm16(cdir / "convert_p225_to_p226_002.wav", a[1])
    write_pcm16(cdir / "convert_p225_to_p226_009.wav", a[2])           # no reference
    write_pcm16(rdir / "p226_001.wav", b[0])
    t48 = np.arange(3 * len(b[1])) / 48000.0
    x48 = (0.3 * np.sin(2 * np.pi * 210 * t48) + 0.1 * np.sin(2 * np.pi * 420 * t48)
           + 0.003 * np.random.RandomState(30).randn(t48.size)).astype(np.float32)
    write_pcm16(rdir / "p226_002.wav", x48, sr=48000)                   # scored through the resampler
    write_pcm16(rdir / "p226_005.wav", b[2])                            # no converted file
    p = _run([cdir, rdir])
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[0].startswith("utterance 001 mcd: ") and lines[1].startswith("utterance 002 mcd: ")
    assert lines[-1].startswith("mean mcd: ")
    res = json.loads((cdir / "mcd.json").read_text())
    assert [r["utterance"] for r in res["pairs"]] == ["001", "002"] and res["scored"] == 2
    assert [os.path.basename(x) for x in res["unmatched"]["converted"]] == ["convert_p225_to_p226_009.wav"]
    assert [os.path.basename(x) for x in res["unmatched"]["reference"]] == ["p226_005.wav"]
    for r, line in zip(res["pairs"], lines):
        assert float(line.split("mcd: ")[1]) == r["mcd"] and r["mcd"] > 0
    assert np.isclose(res["mean_mcd"], np.mean([r["mcd"] for r in res["pairs"]]), rtol=1e-15)
    # the 48 kHz reference scores as the Resampler's output for it does
    c2, _ = read_wav(cdir / "convert_p225_to_p226_002.wav")
    r48, sr = read_wav(rdir / "p226_002.wav")
    assert sr == 48000
    r16 = resample_batch([r48], [sr])[0]
    direct = ev.mcd_batch([c2], [r16], features=fe)
    assert direct["mcd"][0] == res["pairs"][1]["mcd"], (direct["mcd"][0], res["pairs"][1]["mcd"])
    # --json elsewhere, and nothing to pair
    out = tmp_path / "elsewhere.json"
    assert _run([cdir, rdir, "--json", out]).returncode == 0 and json.loads(out.read_text())["scored"] == 2
    empty = tmp_path / "empty"
    empty.mkdir()
    q = _run([cdir, empty])
    assert q.returncode != 0 and json.loads((cdir / "mcd.json").read_text())["pairs"] == []
