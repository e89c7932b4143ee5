"""Corpus preprocessing on the GPU (dvae_amd.preprocess): the resample kernel against the float64 restatement of resampy
kaiser_best (tests/test_preprocess.py), volume normalisation, the segmented mel passes, the pinned mel path, and the CLI end
to end (wav tree -> corpus -> one training epoch)."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dvae_amd  # noqa: E402,F401
from test_preprocess import RATES, normalize_ref, resample_ref, tone  # noqa: E402


def _inputs(sr, seed):
    """noise and tones, lengths from resampy's minimum to ~2 s plus odd tails"""
    rs = np.random.RandomState(seed)
    n_min = -(-sr // 16000)
    lens = [n_min, n_min + 1, 7, 255, 1000 + seed, sr // 2 + 13, 2 * sr + 3]
    out = []
    for i, n in enumerate(lens):
        x = rs.uniform(-1, 1, n) if i % 2 == 0 else 0.8 * tone(n, sr, 440.0 * (i + 1)) + 0.05 * rs.randn(n)
        out.append(x.astype(np.float32))
    return out


@pytest.mark.parametrize("sr", RATES)
def test_resample_matches_the_float64_restatement(sr):
    import torch
    from dvae_amd.preprocess import resample_batch
    xs = _inputs(sr, sr % 97)
    ys = resample_batch(xs, [sr] * len(xs))
    torch.cuda.synchronize()
    for x, y in zip(xs, ys):
        y = y.cpu().numpy()
        f64 = resample_ref(x, sr)
        f32 = resample_ref(x, sr, dtype=np.float32)
        assert y.shape == f64.shape, (len(x), y.shape, f64.shape)
        bound = 4 * np.max(np.abs(f32 - f64)) + 1e-7 * np.max(np.abs(x))
        err = np.max(np.abs(y - f64))
        assert err <= bound, (sr, len(x), err, bound)


def test_same_rate_returns_the_input():
    import torch
    from dvae_amd.preprocess import resample_batch
    x = torch.randn(1001, device="cuda")
    y = resample_batch([x], [16000])[0]
    assert y.data_ptr() == x.data_ptr() and torch.equal(x, y)
    xh = np.random.RandomState(0).randn(77).astype(np.float32)
    assert np.array_equal(resample_batch([xh], [16000])[0].cpu().numpy(), xh)


def test_batch_independence_and_determinism():
    import torch
    from dvae_amd.preprocess import Resampler, resample_batch
    rs = np.random.RandomState(5)
    srs = [48000, 8000, 44100, 22050, 48000, 32000, 24000, 44100]
    xs = [rs.uniform(-1, 1, int(n)).astype(np.float32) for n in rs.randint(3, 40000, len(srs))]
    r = Resampler()
    together = [y.cpu().numpy() for y in resample_batch(xs, srs, resampler=r)]
    again = [y.cpu().numpy() for y in resample_batch(xs, srs, resampler=Resampler())]
    for i, (x, sr) in enumerate(zip(xs, srs)):
        alone = resample_batch([x], [sr])[0].cpu().numpy()
        assert np.array_equal(alone, together[i]), (i, sr)
        assert np.array_equal(again[i], together[i])
    torch.cuda.synchronize()


def test_volume_normalisation():
    import torch
    from dvae_amd.preprocess import normalize_volume_batch
    rs = np.random.RandomState(2)
    quiet = (1e-3 * rs.randn(12345)).astype(np.float32)
    loud = (0.5 * rs.randn(3001)).astype(np.float32)
    tiny = (1e-4 * rs.randn(5)).astype(np.float32)
    silent = np.zeros(4097, dtype=np.float32)
    ys, sil = normalize_volume_batch([quiet, loud, silent, tiny])
    torch.cuda.synchronize()
    assert sil.tolist() == [False, False, True, False]
    for x, y in ((quiet, ys[0]), (tiny, ys[3])):
        _, g = normalize_ref(x)
        got = y.cpu().numpy().astype(np.float64) / x.astype(np.float64)
        assert np.allclose(got, g, rtol=1e-6, atol=0), (got[:3], g)
    assert np.array_equal(ys[1].cpu().numpy(), loud)                 # already louder than -30 dBFS: untouched
    assert np.array_equal(ys[2].cpu().numpy(), silent)


def test_segmented_frames_and_db_equal_the_per_utterance_kernels():
    import torch
    from dvae_amd._lib import check, lib, ptr, stream
    from dvae_amd.frontend import MelFrontend
    fe = MelFrontend()
    L = lib()
    rs = np.random.RandomState(3)
    ns = [1, 255, 256, 4097, 16000 + 5]
    sigs = [torch.from_numpy(rs.uniform(-1, 1, n).astype(np.float32)).cuda() for n in ns]
    ms = [fe.num_frames(n) for n in ns]
    from dvae_amd.packed import segment_table
    from dvae_amd.preprocess import pack
    wav, offs = pack(sigs)
    table = segment_table(ms, offs, ns)
    segs = torch.from_numpy(table).cuda()
    rows = sum(ms)
    seg = torch.empty((rows, fe.fsize), device="cuda")
    check(L.dvae_stft_frames_seg(ptr(wav), ptr(segs), len(ns), rows, ptr(fe.window), ptr(seg), fe.fsize, fe.hop,
                                 fe.fsize - fe.hop, stream()), "seg")
    one = torch.empty_like(seg)
    for s, m, r0 in zip(sigs, ms, table[:, 0]):
        check(L.dvae_stft_frames(ptr(s), s.numel(), ptr(fe.window), one[int(r0):].data_ptr(), m, fe.fsize, fe.hop,
                                 fe.fsize - fe.hop, stream()), "one")
    assert torch.equal(seg, one)
    mel = torch.rand((rows, fe.n_mels), device="cuda") * 3.0
    mel[::7] = 0.0
    out = torch.empty(rows * fe.n_mels, device="cuda")
    check(L.dvae_mel_db_normalize_seg(ptr(mel), ptr(out), ptr(segs), len(ns), rows, fe.n_mels, fe.min_level,
                                      fe.ref_level_db, fe.min_level_db, stream()), "dbseg")
    for m, r0, blk in zip(ms, table[:, 0], fe.unpack(out, ms)):
        ref = torch.empty((fe.n_mels, m), device="cuda")
        check(L.dvae_mel_db_normalize(mel[int(r0):].data_ptr(), ptr(ref), m, fe.n_mels, m, 0, fe.min_level,
                                      fe.ref_level_db, fe.min_level_db, stream()), "db")
        assert torch.equal(blk, ref)


def test_pinned_mel_alone_and_in_a_batch_and_against_float64():
    import torch
    from dvae_amd.frontend import MelFrontend
    from dvae_amd.preprocess import normalize_volume_batch, resample_batch
    from oracle.mel_ref import melspectrogram
    fe = MelFrontend()
    rs = np.random.RandomState(4)
    srs = [48000, 44100, 16000, 22050]
    xs = [(0.01 * rs.randn(int(sr * d)) + 0.02 * tone(int(sr * d), sr, 300.0)).astype(np.float32)
          for sr, d in zip(srs, (1.3, 0.7, 2.1, 0.45))]
    ys = resample_batch(xs, srs)
    ys, sil = normalize_volume_batch(ys)
    assert not sil.any()
    batch = [m.cpu().numpy() for m in fe.melspectrogram_batch(ys, unsplit=True)]
    for i, y in enumerate(ys):
        alone = fe.melspectrogram_batch([y], unsplit=True)[0].cpu().numpy()
        assert np.array_equal(alone, batch[i]), i
        w64, _ = normalize_ref(resample_ref(xs[i], srs[i]))
        want = melspectrogram(w64)
        assert batch[i].shape == want.shape
        assert np.max(np.abs(batch[i] - want)) <= 2e-4, (i, np.max(np.abs(batch[i] - want)))
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------- end to end
def _write_pcm16(path, x, sr, ch=1):
    path.parent.mkdir(parents=True, exist_ok=True)
    v = np.clip(np.round(np.asarray(x) * 32767), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(ch)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(v.tobytes())


def _write_s24(path, x, sr):
    import struct
    v = np.clip(np.round(np.asarray(x) * (2 ** 23 - 1)), -2 ** 23, 2 ** 23 - 1).astype(np.int64)
    data = b"".join(int(s & 0xFFFFFF).to_bytes(3, "little") for s in v)
    fmt = struct.pack("<HHIIHH", 1, 1, sr, sr * 3, 3, 24)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(data)) + data
    body += b"\x00" if len(data) & 1 else b""
    path.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)


def _tree(root):
    rs = np.random.RandomState(9)
    w = root / "VCTK-Corpus" / "wav16"
    speech = lambda n, sr, f: 0.05 * tone(n, sr, f) * (1 + 0.5 * np.sin(np.arange(n) * 7.0 / sr)) + 0.003 * rs.randn(n)
    for s, spk in enumerate(("p225", "p226", "p227")):
        for u in range(4):
            n = int(48000 * (0.6 + 0.15 * u + 0.1 * s))
            _write_pcm16(w / spk / f"{spk}_{u:03d}.wav", speech(n, 48000, 150.0 * (s + 1) + 40 * u), 48000)
    st = np.stack([speech(30000, 44100, 220.0), speech(30000, 44100, 330.0)], 1).ravel()
    _write_pcm16(w / "p225" / "p225_st.wav", st, 44100, ch=2)
    _write_s24(w / "p226" / "p226_s24.wav", speech(20000, 48000, 500.0), 48000)
    _write_pcm16(w / "p227" / "sub" / "p227_n.wav", speech(40000, 48000, 260.0), 48000)
    _write_pcm16(w / "p227" / "p227_silent.wav", np.zeros(24000), 48000)
    _write_pcm16(w / "p226" / "p226_short.wav", np.array([0.1, -0.1]), 48000)
    return w


def _run(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "dvae_amd.preprocess"] + args, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r


def _snapshot(d):
    return {str(p.relative_to(d)): p.read_bytes() for p in sorted(d.rglob("*")) if p.is_file()}


def test_cli_end_to_end_then_train(tmp_path):
    from dvae_amd.preprocess import read_wav
    from oracle.mel_ref import melspectrogram
    root = tmp_path / "data"
    wav16 = _tree(root)
    out = tmp_path / "mel"
    r = _run([str(root), "-o", str(out), "--no_trim", "--workers", "3"])
    summary = r.stdout.strip().splitlines()[-1]
    assert "p227_silent.wav (silent)" in summary and "p226_short.wav (too short" in summary, summary
    assert sorted(p.name for p in out.iterdir()) == ["p225", "p226", "p227"]
    want = {"p225": [f"p225_{u:03d}_mel.npy" for u in range(4)] + ["p225_st_mel.npy"],
            "p226": [f"p226_{u:03d}_mel.npy" for u in range(4)] + ["p226_s24_mel.npy"],
            "p227": [f"p227_{u:03d}_mel.npy" for u in range(4)] + ["sub_p227_n_mel.npy"]}
    for spk, names in want.items():
        got = sorted(p.name for p in (out / spk).glob("*.npy"))
        assert got == sorted(names), (spk, got)
        lines = (out / spk / "_sources.txt").read_text().splitlines()
        assert sorted(l.split(",")[0] for l in lines) == sorted(names)
        for l in lines:
            name, src = l.split(",", 1)
            assert src.startswith(str(wav16 / spk)) and src.endswith(".wav")
            mel = np.load(out / spk / name)
            assert mel.dtype == np.float32 and mel.shape[0] == 80 and mel.min() >= 0 and mel.max() <= 1
            x, sr = read_wav(src)
            w64, _ = normalize_ref(resample_ref(x, sr))
            ref = melspectrogram(w64)
            assert mel.shape == ref.shape
            assert np.max(np.abs(mel - ref)) <= 3e-4, (name, np.max(np.abs(mel - ref)))
    before = _snapshot(out)
    _run([str(root), "-o", str(out), "--no_trim", "-s"])
    assert _snapshot(out) == before                                   # -s: nothing written, nothing changed
    o1, o600 = tmp_path / "b1", tmp_path / "b600"
    _run([str(root), "-o", str(o1), "--no_trim", "--batch-seconds", "1", "--workers", "1"])
    _run([str(root), "-o", str(o600), "--no_trim", "--batch-seconds", "600", "--workers", "16"])
    s1, s600 = _snapshot(o1), _snapshot(o600)
    npys = [k for k in s1 if k.endswith(".npy")]
    assert len(npys) == 15 and sorted(npys) == sorted(k for k in s600 if k.endswith(".npy"))
    assert all(s1[k] == s600[k] == before[k] for k in npys)
    # the corpus trains (test_hip_train_cli.py's pattern)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(PYTHONPATH=ROOT + os.pathsep + env.get("PYTHONPATH", ""))
    log_dir = tmp_path / "results"
    cmd = [sys.executable, "-c", "import dvae_amd.train as t, sys; t.main(sys.argv[1:])", "--train", "true",
           f"--dataset_fp={out}", "--batch-size=2", "--latent-size=32", "--speaker_size=4", "--lr=1e-4", "--epochs=1",
           "--report-interval=1", "--mse_cof=10", "--kl_cof=10", f"--log_dir={log_dir}", "--seed=3", "--do-not-resume"]
    t = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert t.returncode == 0, (t.stdout[-1500:], t.stderr[-3000:])
    recs = [json.loads(l) for l in open(log_dir / "logs" / "DisentangledVAE_VCTK" / "scalars.jsonl")]
    assert [x["epoch"] for x in recs] == [1] and all(v == v for v in recs[0].values())
