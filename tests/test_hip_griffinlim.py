"""Griffin-Lim inverse of the mel front-end on the GPU (frontend.MelInverter, csrc/frontend.hip) against the float64
restatement of tests/test_griffinlim.py, and `train.py --convert` end to end."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from oracle import mel_ref
from test_griffinlim import griffin_lim, linear_magnitude, mel_of, residual, signal, tables

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = mel_ref.HOP_SIZE


@pytest.fixture(scope="module")
def inv():
    from dvae_amd.frontend import MelInverter
    return MelInverter()


@pytest.fixture(scope="module")
def fe():
    from dvae_amd.frontend import MelFrontend
    return MelFrontend()


def _gpu_stft(fe, x):
    """the front-end's own framing + DFT contraction: -> (|D|, angle D) [M, nb] device tensors"""
    from dvae_amd import ops
    from dvae_amd._lib import check, lib, ptr, stream
    s = torch.as_tensor(x).cuda().contiguous()
    M = fe.num_frames(s.numel())
    frames = torch.empty((M, fe.fsize), device="cuda")
    check(lib().dvae_stft_frames(ptr(s), s.numel(), ptr(fe.window), ptr(frames), M, fe.fsize, fe.hop, fe.fsize - fe.hop,
                                 stream()), "dvae_stft_frames")
    reim = ops.linear_fwd(frames, fe.dft_basis, None, mode=ops.MODE_F32)
    re, im = reim[:, :fe.nb], reim[:, fe.nbp:fe.nbp + fe.nb]
    return torch.hypot(re, im), torch.atan2(im, re)


@pytest.mark.parametrize("n", [256, 1000, 4096, 16001, 32000])
def test_hip_inverse_stft_is_exact(inv, fe, n):
    """GPU STFT -> inverse contraction -> overlap-add gather recovers the signal (frame at n, invert at the M it gave)"""
    x = signal(n, n % 5)
    mag, ph = _gpu_stft(fe, x)
    M = mag.shape[0]
    assert inv.num_samples(M) >= n and mel_ref.lws_num_frames(inv.num_samples(M)) == M
    y = inv.griffinlim_batch([mag], n_iter=0, init_phase=[ph])[0].cpu().numpy()
    assert y.shape == (inv.num_samples(M),)
    err = np.abs(y[:n] - x).max()
    print(f"n={n}: max |x - istft(stft(x))| = {err:.2e}")
    assert err <= 1e-5
    assert np.abs(y[n:]).max(initial=0.0) <= 1e-5          # the zero padding beyond n comes back as zeros


def test_hip_linear_magnitude_solve(inv):
    tb = tables()
    for seed in (1, 4):
        mel = mel_of(signal(32000, seed))
        got = inv.linear_magnitude_batch([mel.astype(np.float32)])[0].cpu().numpy()
        assert got.shape == (mel.shape[1], tb["nb"]) and got.min() >= 0.0
        ref = linear_magnitude(mel, 200, tb)
        rg, rr = residual(got, mel, tb), residual(ref, mel, tb)
        print(f"seed {seed}: residual median GPU {np.median(rg):.2e}, fp64 {np.median(rr):.2e}, worst ratio "
              f"{np.max(rg / (rr + 1e-12)):.3f}")
        assert np.all(rg <= 1.5 * rr + 1e-5)


@pytest.mark.parametrize("n_iter", [1, 4, 32])
def test_hip_griffin_lim_against_fp64(inv, n_iter):
    """same magnitude, same initial phase: the GPU waveform is as close to float64 as float32 numpy is (x3, floor 1e-5)"""
    tb = tables()
    mel = mel_of(signal(32000, 3))
    S = inv.linear_magnitude_batch([mel.astype(np.float32)])[0].cpu().numpy().astype(np.float64)
    ph = 2 * np.pi * np.random.RandomState(7).random_sample(S.shape)
    got = inv.griffinlim_batch([S], n_iter=n_iter, init_phase=[ph])[0].cpu().numpy().astype(np.float64)
    ref = griffin_lim(S, ph, n_iter, tb=tb)
    r32 = griffin_lim(S.astype(np.float32), ph.astype(np.float32), n_iter, dtype=np.float32, tb=tb).astype(np.float64)
    d_gpu = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    d_32 = np.linalg.norm(r32 - ref) / np.linalg.norm(ref)
    bound = max(1e-5, 3.0 * d_32)
    print(f"n_iter={n_iter}: GPU {d_gpu:.2e}, numpy fp32 {d_32:.2e}, ratio {d_gpu / max(d_32, 1e-30):.2f}")
    assert d_gpu <= bound


def test_hip_round_trip_mel_wav_mel(inv, fe):
    """MelFrontend -> MelInverter -> MelFrontend"""
    for seed in (1, 3, 4):
        mel = fe.melspectrogram(signal(32000, seed))
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        wav = inv.waveform(mel, generator=g)
        back = fe.melspectrogram(wav)
        assert back.shape == mel.shape
        d = (back - mel).abs().flatten()
        mean, p99 = float(d.mean()), float(torch.quantile(d, 0.99))
        print(f"seed {seed}: re-mel mean |d| {mean:.4f}, p99 {p99:.4f}")
        assert mean <= 0.01 and p99 <= 0.06


def test_hip_round_trip_tracks_the_restatement():
    """Signal 5 is harder for Griffin-Lim itself: the float64 restatement reaches a p99 of ~0.085 on it (signals 1 / 3 / 4:
    0.04 .. 0.05).  Same phase on both sides: the GPU's round trip is as good as float64's."""
    from dvae_amd.frontend import MelFrontend, MelInverter
    fe, inv = MelFrontend(), MelInverter()
    tb = tables()
    mel64 = mel_of(signal(32000, 5))
    ph = 2 * np.pi * np.random.RandomState(5).random_sample((mel64.shape[1], tb["nb"]))
    ref = np.abs(mel_of(griffin_lim(linear_magnitude(mel64, 200, tb), ph, 32, tb=tb)) - mel64)
    mel = fe.melspectrogram(signal(32000, 5))
    got = (fe.melspectrogram(inv.waveform(mel, init_phase=[ph])) - mel).abs().cpu().numpy()
    print(f"signal 5: re-mel mean |d| GPU {got.mean():.4f} fp64 {ref.mean():.4f}; p99 GPU "
          f"{np.quantile(got, 0.99):.4f} fp64 {np.quantile(ref, 0.99):.4f}")
    assert got.mean() <= 0.01 and got.mean() <= 1.1 * ref.mean()
    assert np.quantile(got, 0.99) <= 1.15 * np.quantile(ref, 0.99)


def test_hip_batching_and_determinism(inv, fe):
    from dvae_amd import ops
    mels = [fe.melspectrogram(signal(n, i)) for i, n in enumerate((16000, 7000, 24577))]
    phases = [2 * np.pi * np.random.RandomState(i).random_sample((m.shape[1], inv.nb)) for i, m in enumerate(mels)]
    kw = dict(n_iter=8)
    batch = [w.clone() for w in inv.waveform_batch(mels, init_phase=phases, **kw)]
    for m, p, b in zip(mels, phases, batch):
        one = inv.waveform_batch([m], init_phase=[p], **kw)[0]
        assert one.shape == b.shape == (inv.num_samples(m.shape[1]),)
        assert torch.equal(one, b)
    again = inv.waveform_batch(mels, init_phase=phases, **kw)
    assert all(torch.equal(a, b) for a, b in zip(again, batch))
    zeros = [w.clone() for w in inv.waveform_batch(mels, init="zeros", **kw)]
    prev, prev_det = ops.get_compute_dtype(), ops.deterministic()
    try:
        for mode in ("bf16", "fp32", "fp32x3"):
            with ops.compute_dtype(mode):
                got = inv.waveform_batch(mels, init="zeros", **kw)
            assert all(torch.equal(a, b) for a, b in zip(got, zeros)), mode
        ops.set_deterministic(True)
        got = inv.waveform_batch(mels, init="zeros", **kw)
        assert all(torch.equal(a, b) for a, b in zip(got, zeros))
    finally:
        ops.set_deterministic(prev_det)
        ops.set_compute_dtype(prev)
    g1, g2 = torch.Generator(device="cuda"), torch.Generator(device="cuda")
    g1.manual_seed(5)
    g2.manual_seed(5)
    assert torch.equal(inv.waveform(mels[1], generator=g1, n_iter=2), inv.waveform(mels[1], generator=g2, n_iter=2))
    with pytest.raises(ValueError):
        inv.waveform(mels[0][:, :3])
    with pytest.raises(ValueError):
        inv.waveform_batch([mels[0], mels[1][:, :2]])
    from dvae_amd._lib import lib
    tab = np.zeros((1, 4), dtype=np.int64)
    assert lib().dvae_gl_segment_table(np.array([3], dtype=np.int32).ctypes.data, 1, 1024, 256, tab.ctypes.data) != 0
    assert lib().dvae_gl_segment_table(np.array([4], dtype=np.int32).ctypes.data, 1, 1024, 256, tab.ctypes.data) == 0
    assert list(tab[0]) == [0, 4, 0, 256]


def test_hip_convert_cli_writes_wavs(tmp_path, fe):
    import dvae_amd
    corpus = tmp_path / "corpus"
    for s, spk in enumerate(("spkA", "spkB")):
        (corpus / spk).mkdir(parents=True)
        wavs = [signal(20000 + 3000 * u + 500 * s, 10 * s + u) for u in range(3)]
        for u, mel in enumerate(fe.melspectrogram_batch(wavs)):
            np.save(corpus / spk / f"{spk}_u{u}_mel.npy", mel.cpu().numpy())
    log_dir = tmp_path / "results"
    (log_dir / "checkpoints").mkdir(parents=True)
    torch.manual_seed(0)
    vsc = dvae_amd.ConvolutionalMulVAE("VCTK", 64, 80, 32, 1e-4, 0.01, 500, False, batch_size=2, speaker_size=4,
                                       device=torch.device("cuda"), latent_dim=32)
    torch.save(vsc.model.state_dict(), log_dir / "checkpoints" / "DisentangledVAE_VCTK_0.pth")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, "-c", "import dvae_amd.train as t, sys; t.main(sys.argv[1:])", "--convert", "True",
           f"--dataset_fp={corpus}", f"--log_dir={log_dir}", "--src_spk=spkA", "--trg_spk=spkB", "--seed=4",
           "--batch-size=2", "--latent-size=32", "--speaker_size=4"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    out = log_dir / "generation" / "spkA_to_spkB"
    srcs = sorted((corpus / "spkA").glob("*.npy"))[:2]
    trgs = sorted((corpus / "spkB").glob("*.npy"))
    rng = np.random.RandomState(4)
    vsc.model.load_state_dict(torch.load(log_dir / "checkpoints" / "DisentangledVAE_VCTK_0.pth", map_location="cuda"))
    for fp in srcs:
        utt = fp.stem.split("_")[-2]
        tfp = trgs[rng.randint(len(trgs))]
        for name in (f"source_spkA_{utt}.npy", f"recons_spkA_{utt}.npy"):
            assert (out / name).exists(), name
        conv = np.load(out / f"convert_spkA_to_spkB_{utt}.npy")
        want = vsc.convert_mel(np.load(fp), np.load(tfp))["converted"].cpu().numpy()
        assert conv.shape == want.shape and np.abs(conv - want).max() <= 1e-6
        n_chunks = np.load(fp).shape[1] // 64 + 1
        assert conv.shape == (80, n_chunks * 64)
        with wave.open(str(out / f"convert_spkA_to_spkB_{utt}.wav"), "rb") as w:
            assert (w.getframerate(), w.getnchannels(), w.getsampwidth()) == (16000, 1, 2)
            assert w.getnframes() == (n_chunks * 64 - 3) * HOP
            pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.float32) / 32767.0
        back = fe.melspectrogram(pcm).cpu().numpy()
        d = np.abs(back - conv).mean()
        print(f"{utt}: re-mel of the .wav vs converted mel: mean |d| {d:.4f}")
        assert d <= 0.03
