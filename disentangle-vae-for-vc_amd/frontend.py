"""Mel front-end on the GPU: waveform -> [80, M] normalised log-mel, the array format the training
corpus stores as `<speaker>/*.npy` and `SpeechDatasetGVAE` / `GpuPairLoader` consume.

Mirrors /root/reference/preprocessing/utils.py:68-73 `melspectrogram(y)` with preprocessing/hparams.py:58-80
(16 kHz, fft 1024, hop 256, 80 mels, 90-7600 Hz, min_level_db -100, ref_level_db 16, clipping allowed):

    D = lws.lws(1024, 256, mode="speech").stft(y).T ; S = 20*log10(max(1e-5, mel_basis @ |D|)) - 16
    return clip((S + 100) / 100, 0, 1)

MI355X formulation: every frame of every utterance of a batch is one row of a `[sum M, 1024]` matrix; the STFT is ONE
fp32 contraction against a precomputed `[2*516, 1024]` cos/-sin basis (one-sided spectrum, 513 bins padded to 516 so
that rows stay 16-byte aligned), the mel projection a second one against `[80, 516]`, both on `dvae_gemm_f32` (MFMA);
framing+window, magnitude and dB/normalise/transpose are three HBM-bound HIP passes (`csrc/frontend.hip`).
The window and the two bases are built on the host in float64 (they are constants of the hyper-parameters):
`lws` and `librosa` are NOT dependencies — their published constructions are restated here (see oracle/mel_ref.py
for the parity status of exactly these two pieces).  No CPU fallback: CPU tensors are moved to the device.

`MelInverter` is the way back (normalised mel -> waveform: non-negative mel -> linear solve and fast Griffin-Lim on the
same window and bases, `inverse_tables`).
"""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np
import torch

from . import ops
from ._lib import check, lib, ptr, stream
from .packed import (flat, hann_periodic, onesided_dft, pack, pack_rows, padded_bins, pinned_gemm, segment_table,
                     split_rows, upload)


def _slaney_hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-30) / 1000.0) / (np.log(6.4) / 27.0), f * 3.0 / 200.0)


def _slaney_mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), m * 200.0 / 3.0)


def lws_window(fft_size: int, hop_size: int) -> np.ndarray:
    """lws "speech" analysis (and synthesis) window: sqrt(periodic Hann * 2*hop/fsize), float64 [fsize]."""
    return np.sqrt(hann_periodic(fft_size) * 2.0 * hop_size / fft_size)


def dft_basis(fft_size: int, nbp: int) -> np.ndarray:
    """One-sided forward DFT basis, float64 [2*nbp, fsize]: rows [0, nb) cos, rows [nbp, nbp+nb) -sin, padded bins 0."""
    nb = fft_size // 2 + 1
    cos, sin = onesided_dft(fft_size)
    basis = np.zeros((2 * nbp, fft_size), dtype=np.float64)
    basis[:nb] = cos.T
    basis[nbp:nbp + nb] = -sin.T
    return basis


def mel_basis(sample_rate: int, fft_size: int, num_mels: int, fmin: float, fmax: float, nbp: int) -> np.ndarray:
    """librosa.filters.mel (htk=False, Slaney area normalisation), float64 [num_mels, nbp] (padded bins 0)."""
    nb = fft_size // 2 + 1
    fft_f = np.linspace(0.0, sample_rate / 2.0, nb)
    mel_f = _slaney_mel_to_hz(np.linspace(_slaney_hz_to_mel(fmin), _slaney_hz_to_mel(fmax), num_mels + 2))
    lower = (fft_f[None, :] - mel_f[:-2, None]) / (mel_f[1:-1] - mel_f[:-2])[:, None]
    upper = (mel_f[2:, None] - fft_f[None, :]) / (mel_f[2:] - mel_f[1:-1])[:, None]
    melw = np.zeros((num_mels, nbp), dtype=np.float64)
    melw[:, :nb] = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]
    return melw


class MelFrontend:
    def __init__(self, device="cuda", sample_rate=16000, fft_size=1024, hop_size=256, num_mels=80, fmin=90.0,
                 fmax=7600.0, min_level_db=-100.0, ref_level_db=16.0):
        if fft_size % 4 or hop_size < 1 or hop_size > fft_size:
            raise ValueError("MelFrontend: fft_size must be a multiple of 4 and 1 <= hop_size <= fft_size")
        if not fmax <= sample_rate / 2:
            raise ValueError("MelFrontend: fmax above Nyquist")            # utils.py:115
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("MelFrontend runs on the HIP path only (no CPU fallback)")
        self.sr, self.fsize, self.hop, self.n_mels = sample_rate, fft_size, hop_size, num_mels
        self.min_level_db, self.ref_level_db = float(min_level_db), float(ref_level_db)
        self.min_level = float(np.exp(min_level_db / 20.0 * np.log(10.0)))  # utils.py:128
        nb = fft_size // 2 + 1
        self.nb, self.nbp = nb, padded_bins(fft_size)
        self.window = upload(lws_window(fft_size, hop_size), self.device)
        self.dft_basis = upload(dft_basis(fft_size, self.nbp), self.device)
        self.mel_basis = upload(mel_basis(sample_rate, fft_size, num_mels, fmin, fmax, self.nbp), self.device)
        self.mode = ops.MODE_F32

    # ---- utils.py:82-103
    def num_frames(self, length: int) -> int:
        pad = self.fsize - self.hop
        extra = 1 if length % self.hop == 0 else 2
        return (length + 2 * pad - self.fsize) // self.hop + extra

    def melspectrogram_batch(self, wavs: Sequence, unsplit: bool = False) -> list:
        """List of 1-D waveforms (numpy / tensors, any length >= 1) -> list of device tensors [80, M_i] (views of one
        packed buffer).  unsplit=True: the pinned path of the corpus tool (preprocess.py): both contractions with ONE
        k-split, so that an utterance's mel is bit-identical whatever batch it lands in (the default lets the
        contraction pick a split from the row count)."""
        sigs = [flat(w) for w in wavs]
        wav, offs = pack(sigs, self.device)
        return self.unpack(*self.mel_packed(wav, offs, [s.shape[0] for s in sigs], pinned=unsplit))

    def _contract(self, A, B, K, pinned):
        # features must not depend on the training compute mode (bf16 would put a leakage floor ~50 dB under each frame's
        # peak against a 100 dB normalisation range): exact fp32 products either way; only the k-split differs
        if not pinned:
            return ops.linear_fwd(A, B, None, mode=self.mode)
        C = torch.empty((A.shape[0], B.shape[0]), device=self.device, dtype=torch.float32)
        pinned_gemm(A, B, C, K)
        return C

    def mel_packed(self, wav, sample0, lengths, pinned=True):
        """Mel of the signals wav[sample0[i], sample0[i] + lengths[i]) of one device buffer: five launches for the whole
        batch -> (packed out: the [80, M_i] blocks back to back, [M_i]).  `pinned` selects how the two contractions run
        and nothing else."""
        L = lib()
        ns = [int(n) for n in lengths]
        if not ns or min(ns) < 1:
            raise ValueError("melspectrogram: empty waveform")
        ms = [self.num_frames(n) for n in ns]
        segs = upload(segment_table(ms, sample0, ns), self.device, np.int64)
        rows = int(sum(ms))
        frames = torch.empty((rows, self.fsize), device=self.device, dtype=torch.float32)
        check(L.dvae_stft_frames_seg(ptr(wav), ptr(segs), len(ns), rows, ptr(self.window), ptr(frames), self.fsize,
                                     self.hop, self.fsize - self.hop, stream()), "dvae_stft_frames_seg")
        reim = self._contract(frames, self.dft_basis, self.fsize, pinned)        # [rows, 2*nbp]
        del frames
        mag = torch.empty((rows, self.nbp), device=self.device, dtype=torch.float32)
        check(L.dvae_stft_magnitude(ptr(reim), ptr(mag), rows, self.nbp, stream()), "dvae_stft_magnitude")
        del reim
        mel = self._contract(mag, self.mel_basis, self.nbp, pinned)             # [rows, 80]
        out = torch.empty(rows * self.n_mels, device=self.device, dtype=torch.float32)
        check(L.dvae_mel_db_normalize_seg(ptr(mel), ptr(out), ptr(segs), len(ns), rows, self.n_mels, self.min_level,
                                          self.ref_level_db, self.min_level_db, stream()), "dvae_mel_db_normalize_seg")
        return out, ms

    def unpack(self, out, ms):
        """packed [80, M_i] blocks (a device or host tensor / array) -> list of [80, M_i] views"""
        return [blk.reshape(self.n_mels, m) for blk, m in zip(split_rows(out, [self.n_mels * m for m in ms]), ms)]

    def melspectrogram(self, wav):
        """One waveform -> [80, M] in [0, 1] (utils.py:68-73)."""
        return self.melspectrogram_batch([wav])[0]


# ------------------------------------------------------------------------------------------- inverse (mel -> waveform)
def inverse_tables(sample_rate=16000, fft_size=1024, hop_size=256, num_mels=80, fmin=90.0, fmax=7600.0) -> dict:
    """Host-side constants of the Griffin-Lim inverse (float64), built from the same window and mel basis as MelFrontend:
      window     [fsize]           the lws synthesis window (== analysis window)
      mel_basis  [num_mels, nbp]   the forward mel projection M
      inv_basis  [fsize, 2*nbp]    one-sided inverse DFT: y[k] = sum_j c_j/N (Re_j cos - Im_j sin)(2 pi j k / N),
                                   c_0 = c_{N/2} = 1, c_j = 2 otherwise, padded bins 0
      pinv       [nbp, num_mels]   pinv(M): the warm start max(0, A pinv^T) of the non-negative mel -> linear solve
      step       float             1 / ||M||_2^2, the projected-gradient step
      filt_range [num_mels, 2]     per filter its bin range [lo, hi)
      bin_filt   [nbp, 2] int32    per bin at most two filters (-1: none) ...
      bin_w      [nbp, 2]          ... and their weights (Slaney triangles overlap their neighbours only)
      ola_norm   bool              the squared window does NOT overlap-add to 1 at this hop: divide by the envelope"""
    nb, nbp = fft_size // 2 + 1, padded_bins(fft_size)
    win = lws_window(fft_size, hop_size)
    melw = mel_basis(sample_rate, fft_size, num_mels, fmin, fmax, nbp)
    cos, sin = onesided_dft(fft_size, inverse=True)                                  # [fsize, nb]
    inv = np.zeros((fft_size, 2 * nbp), dtype=np.float64)
    inv[:, :nb] = cos
    inv[:, nbp:nbp + nb] = -sin
    pinv = np.linalg.pinv(melw)
    step = 1.0 / float(np.linalg.norm(melw, 2)) ** 2
    rng = np.zeros((num_mels, 2), dtype=np.int32)
    bin_filt = np.full((nbp, 2), -1, dtype=np.int32)
    bin_w = np.zeros((nbp, 2), dtype=np.float64)
    cnt = np.zeros(nbp, dtype=np.int64)
    for f in range(num_mels):
        nz = np.nonzero(melw[f])[0]
        if nz.size:
            rng[f] = (nz[0], nz[-1] + 1)
            assert np.all(melw[f, nz[0]:nz[-1] + 1] > 0), "a mel filter with a gap"
        for j in nz:
            assert cnt[j] < 2, f"bin {j} under more than two mel filters"
            bin_filt[j, cnt[j]], bin_w[j, cnt[j]] = f, melw[f, j]
            cnt[j] += 1
    if fft_size % hop_size:
        raise ValueError("inverse_tables: fft_size must be a multiple of hop_size")
    # steady-state overlap-add of the squared window (every output sample of the inverse is in the steady state, see
    # MelInverter): 1 for the lws window at hop = fsize/4, so the defaults need no division
    env = (win ** 2).reshape(fft_size // hop_size, hop_size).sum(0)
    ola_norm = not np.allclose(env, 1.0, rtol=0, atol=1e-12)
    return dict(window=win, mel_basis=melw, inv_basis=inv, pinv=pinv, step=step, filt_range=rng, bin_filt=bin_filt,
                bin_w=bin_w, ola_norm=ola_norm, nb=nb, nbp=nbp)


class MelInverter:
    """Normalised mel [80, M] -> waveform of n = (M - 3) * hop samples (lws_num_frames(n) == M), on the GPU:

      amplitude   A = 10^((clip(S, 0, 1) * 100 - 100 + 16) / 20), frame-major       (dvae_mel_denormalize)
      magnitude   X = max(0, A pinv(M)^T), then `nnls_iter` projected-gradient steps
                  X <- max(0, X - eta M^T (M X - A)), one frame per workgroup on chip   (dvae_gemm_f32 + dvae_mel_nnls_pg)
      phase       fast Griffin-Lim (librosa.griffinlim, momentum 0.99) from a random, zero or given phase; per iteration
                  inverse DFT [rows, 2*nbp] x [fsize, 2*nbp]^T, overlap-add + re-framing gather, forward DFT
                  [rows, fsize] x [2*nbp, fsize]^T, fused phase update: four launches for the whole batch
      waveform    a last inverse DFT and the overlap-add gather into the packed output

    The intent of the reference's `simple_inverse` (preprocessing/processing.py:133-139) carried out properly: the front-end
    the corpus was made with is inverted, dB normalisation included.  A batch of utterances of different lengths is packed
    row-wise; only the overlap-add crosses rows, through a small device segment table.  Both DFT contractions are pinned
    to fp32 products and an unsplit k (a row's result does not depend on the training compute mode, the deterministic
    switch or what else shares the batch).  GPU only, no CPU fallback."""

    def __init__(self, device="cuda", sample_rate=16000, fft_size=1024, hop_size=256, num_mels=80, fmin=90.0,
                 fmax=7600.0, min_level_db=-100.0, ref_level_db=16.0, n_iter=32, momentum=0.99, nnls_iter=200):
        if fft_size % 4 or hop_size % 4 or hop_size < 4 or hop_size > fft_size or fft_size % hop_size:
            raise ValueError("MelInverter: fft_size and hop_size must be multiples of 4, fft_size a multiple of hop_size")
        if not fmax <= sample_rate / 2:
            raise ValueError("MelInverter: fmax above Nyquist")
        if not min_level_db < 0:
            raise ValueError("MelInverter: min_level_db must be negative")
        if n_iter < 0 or nnls_iter < 0 or not 0.0 <= momentum:
            raise ValueError("MelInverter: n_iter, nnls_iter and momentum must be >= 0")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("MelInverter runs on the HIP path only (no CPU fallback)")
        self.sr, self.fsize, self.hop, self.n_mels = sample_rate, fft_size, hop_size, num_mels
        self.min_level_db, self.ref_level_db = float(min_level_db), float(ref_level_db)
        self.n_iter, self.momentum, self.nnls_iter = int(n_iter), float(momentum), int(nnls_iter)
        self.min_frames = fft_size // hop_size
        t = inverse_tables(sample_rate, fft_size, hop_size, num_mels, fmin, fmax)
        self.nb, self.nbp, self.step, self.ola_norm = t["nb"], t["nbp"], float(t["step"]), int(t["ola_norm"])
        f32 = lambda a: upload(a, self.device)
        i32 = lambda a: upload(a, self.device, np.int32)
        self.window, self.inv_basis, self.pinv = f32(t["window"]), f32(t["inv_basis"]), f32(t["pinv"])
        self.dft_basis = f32(dft_basis(fft_size, self.nbp))
        self.filt_range, self.bin_filt, self.bin_w = i32(t["filt_range"]), i32(t["bin_filt"]), f32(t["bin_w"])

    def num_samples(self, frames: int) -> int:
        """M frames -> n samples, with lws_num_frames(n) == M"""
        return (frames - self.min_frames + 1) * self.hop

    def _frames_of(self, counts):
        if not counts:
            raise ValueError("MelInverter: empty batch")
        bad = [m for m in counts if m < self.min_frames]
        if bad:
            raise ValueError(f"MelInverter: {bad[0]} frames; the inverse needs >= {self.min_frames} (fft_size / hop_size)")

    def _magnitude(self, mels):
        """list of [80, M_i] -> (X [rows, nbp] device, [M_i])"""
        L = lib()
        ms = [torch.as_tensor(m).to(self.device, torch.float32) for m in mels]
        if any(m.dim() != 2 or m.shape[0] != self.n_mels for m in ms):
            raise ValueError(f"MelInverter: mels must be [{self.n_mels}, M]")
        counts = [int(m.shape[1]) for m in ms]
        self._frames_of(counts)
        mel = torch.cat(ms, dim=1).contiguous() if len(ms) > 1 else ms[0].contiguous()
        rows = mel.shape[1]
        amp = torch.empty((rows, self.n_mels), device=self.device, dtype=torch.float32)
        check(L.dvae_mel_denormalize(ptr(mel), ptr(amp), rows, self.n_mels, rows, self.ref_level_db, self.min_level_db,
                                     stream()), "dvae_mel_denormalize")
        x = torch.empty((rows, self.nbp), device=self.device, dtype=torch.float32)
        pinned_gemm(amp, self.pinv, x, self.n_mels, act=ops.ACT_RELU)
        check(L.dvae_mel_nnls_pg(ptr(amp), ptr(x), rows, self.nbp, self.n_mels, ptr(self.filt_range), ptr(self.bin_filt),
                                 ptr(self.bin_w), self.step, self.nnls_iter, stream()), "dvae_mel_nnls_pg")
        return x, counts

    def linear_magnitude_batch(self, mels: Sequence) -> list:
        """list of [80, M_i] normalised mels -> list of device tensors [M_i, fft_size//2 + 1] (frame-major |STFT|)"""
        x, counts = self._magnitude(mels)
        return split_rows(x[:, :self.nb], counts)

    def griffinlim_batch(self, mags: Sequence, n_iter=None, init="random", generator=None, init_phase=None) -> list:
        """list of [M_i, nb] (or [M_i, nbp]) linear magnitudes -> list of 1-D device waveforms of num_samples(M_i).
        init: "random" (uniform phase from `generator`, or the device's default generator) | "zeros"; init_phase: list of
        [M_i, nb] phases in radians (overrides `init`)."""
        L = lib()
        n_iter = self.n_iter if n_iter is None else int(n_iter)
        if n_iter < 0:
            raise ValueError("MelInverter: n_iter must be >= 0")
        ms = [torch.as_tensor(m).to(self.device, torch.float32) for m in mags]
        counts = [int(m.shape[0]) for m in ms]
        self._frames_of(counts)
        rows, nbp, fs = sum(counts), self.nbp, self.fsize
        if any(m.dim() != 2 or m.shape[1] not in (self.nb, nbp) for m in ms):
            raise ValueError(f"MelInverter: magnitudes must be [M, {self.nb}]")
        S = pack_rows(ms, nbp, self.device)[0]
        phase = None
        if init_phase is not None:
            ps = [torch.as_tensor(p).to(self.device, torch.float32) for p in init_phase]
            if [int(p.shape[0]) for p in ps] != counts:
                raise ValueError("MelInverter: init_phase rows differ from the magnitudes'")
            phase = pack_rows(ps, nbp, self.device)[0]
        elif init == "random":
            gdev = generator.device if generator is not None else self.device
            phase = (2.0 * math.pi) * torch.rand((rows, nbp), generator=generator, device=gdev, dtype=torch.float32)
            phase = phase.to(self.device)
        elif init != "zeros":
            raise ValueError(f"MelInverter: init={init!r}, expected 'random' or 'zeros'")
        table = np.zeros((len(counts), 4), dtype=np.int64)
        cnt = np.asarray(counts, dtype=np.int32)
        check(L.dvae_gl_segment_table(cnt.ctypes.data, len(counts), fs, self.hop, table.ctypes.data),
              "dvae_gl_segment_table")
        segs = torch.from_numpy(table).to(self.device)
        n_total = int(table[-1, 2] + table[-1, 3])
        X = torch.empty((rows, 2 * nbp), device=self.device, dtype=torch.float32)
        check(L.dvae_gl_init(ptr(S), ptr(phase), ptr(X), rows, nbp, stream()), "dvae_gl_init")
        y = torch.empty((rows, fs), device=self.device, dtype=torch.float32)
        frames = torch.empty_like(y)
        reb, prev = torch.empty_like(X), torch.empty_like(X)
        nseg = len(counts)
        for it in range(n_iter):
            pinned_gemm(X, self.inv_basis, y, 2 * nbp)
            check(L.dvae_ola_gather(ptr(y), ptr(segs), nseg, rows, ptr(self.window), ptr(frames), 0, fs, self.hop, 0,
                                    self.ola_norm, stream()), "dvae_ola_gather")
            pinned_gemm(frames, self.dft_basis, reb, fs)
            check(L.dvae_gl_phase(ptr(reb), ptr(prev) if it else None, ptr(S), ptr(X), rows, nbp, self.momentum, stream()),
                  "dvae_gl_phase")
            reb, prev = prev, reb
        pinned_gemm(X, self.inv_basis, y, 2 * nbp)
        wav = torch.empty(n_total, device=self.device, dtype=torch.float32)
        check(L.dvae_ola_gather(ptr(y), ptr(segs), nseg, rows, ptr(self.window), ptr(wav), n_total, fs, self.hop, 1,
                                self.ola_norm, stream()), "dvae_ola_gather")
        return [wav[int(s0):int(s0 + n)] for s0, n in zip(table[:, 2], table[:, 3])]

    def waveform_batch(self, mels: Sequence, n_iter=None, init="random", generator=None, init_phase=None) -> list:
        """list of [80, M_i] normalised mels (the corpus layout) -> list of 1-D device waveforms of (M_i - 3) * hop samples"""
        x, counts = self._magnitude(mels)
        return self.griffinlim_batch(split_rows(x, counts), n_iter=n_iter, init=init, generator=generator, init_phase=init_phase)

    def waveform(self, mel, **kw):
        """One [80, M] mel -> 1-D device waveform"""
        return self.waveform_batch([mel], **kw)[0]
