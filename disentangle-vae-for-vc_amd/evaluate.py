"""Mel-cepstral distortion (MCD) of converted speech on the GPU: the reference's last step,
preprocessing/MCD_calculate.py:54-103 `evaluate_mcd_wav`:

    python -m dvae_amd.evaluate <converted_dir> <reference_dir> [--json PATH] [--f0]

The reference loads both waveforms at 16 kHz, runs WORLD (Harvest F0 at a 5 ms frame period, CheapTrick, then
`pysptk.sp2mc` to order 35 with alpha = mcepalpha(16000)), keeps coefficients [:, :24] of the voiced frames (f0 > 0),
aligns them with fastdtw under the euclidean distance and reports mean(10/ln10 * sqrt(2 * sum diff^2)) along the path.
pyworld, pysptk, fastdtw and librosa are absent, so the score is defined here and is UNPINNED against them
(DESIGN.md §0, f-6): absolute values do not match published WORLD-based MCDs; the score compares runs of this project.

    input      mono 16 kHz; other rates through preprocess.Resampler (resampy kaiser_best, as librosa.load(sr=16000))
    frames     frame k centred on sample 80 k, n // 80 + 1 of them, 512-sample periodic Hann, zero outside the signal
    spectrum   1024-point DFT of the zero-padded frame (one fp32 contraction), P = Re^2 + Im^2, logP = ln(max(P, 1e-10))
    mcep       pysptk.sp2mc restated: c = irfft(logP), c[0] /= 2, SPTK freqt to order 35, alpha 0.41: ONE float64-built
               [36, 513] matrix applied as one contraction; coefficients [:24] (c0 included)
    voicing    (replaces f0 > 0) autocorrelation r from P (one contraction, lags 0 and 20..225 = 16000/800 .. 16000/71),
               r_n = (r / r(0)) / (r_w / r_w(0)) with r_w the window's; voiced iff max r_n >= 0.45 and
               r(0) >= 1e-3 * max r(0) over the utterance (and r(0) > 0)
    alignment  exact DTW (not fastdtw's approximation): steps (i-1,j), (i,j-1), (i-1,j-1) adding d(i,j), a tie to the
               first in that order; the path length rides along with the cost
    MCD        10/ln10 * sqrt(2) * cost / length (float64, host); a side without voiced frames gives NaN, reported and
               left out of the mean (the reference would raise inside fastdtw)

--f0 (replaces Harvest's F0 and `logf0_statistics`, preprocessing/WORLD_processing.py:29-38, :178-185;
UNPINNED against pyworld in the same way) adds, from the same autocorrelation and the same flags:

    f0         per run of voiced frames a Viterbi pass over the 206 lags in float64: local score r_n - OCTAVE_COST per
               octave of lag, JUMP_COST per octave between consecutive frames' lags (Praat's constants), the first maximum
               on a tie; a parabolic refinement of the lag; f0 = 16000 / lag, 0 on unvoiced frames
    lf0 rmse   sqrt(mean (ln f0_x - ln f0_y)^2) over the cells of the MCD's own DTW path, printed in cents
    statistics mean and standard deviation of ln f0 over the voiced frames, per file and pooled per side

Every utterance of a batch is packed row-wise (packed.pack) and runs in one launch per pass; the contractions are pinned
to fp32 and one k-split (packed.pinned_gemm), so an utterance's features and a pair's score are bit-identical
whatever else shares the batch.  GPU only, no CPU fallback.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path
from typing import Sequence

import numpy as np
import torch

from . import packed
from ._lib import check, lib, ptr, stream
from .frontend import dft_basis
from .packed import flat, onesided_dft, pack, pack_rows, pad4, padded_bins, pinned_gemm, segment_table, upload
from .preprocess import Resampler, read_wav, resample_batch

SAMPLE_RATE = 16000
HOP = 80                      # 5 ms
FRAME = 512                   # analysis window (periodic Hann)
FFT_SIZE = 1024               # zero-padded DFT
ORDER = 35                    # sp2mc order (num_mcep 36)
ALPHA = 0.41                  # pysptk.util.mcepalpha(16000)
DIM = 24                      # DVAE_MCD_DIM: coefficients kept, c0 included
POWER_FLOOR = 1e-10
F0_MIN, F0_MAX = 71.0, 800.0
LAG_MIN = int(math.ceil(SAMPLE_RATE / F0_MAX))    # 20
LAG_MAX = int(SAMPLE_RATE // F0_MIN)              # 225
VOICED_PEAK = 0.45            # max normalised autocorrelation of a voiced frame
VOICED_REL_POWER = 1e-3       # r(0) of a voiced frame relative to the utterance's loudest
DTW_MAX_SHORT = 4096          # DVAE_DTW_MAX_SHORT: min(N, M) the DTW kernel supports (20 s of voiced frames)
MCD_SCALE = 10.0 / math.log(10.0) * math.sqrt(2.0)
F0_STATES = LAG_MAX - LAG_MIN + 1                 # DVAE_F0_STATES: state j of the F0 tracker is lag LAG_MIN + j
F0_BACK_LD = 208              # DVAE_F0_BACK_LD: bytes per frame of the back-pointer scratch
OCTAVE_COST = 0.01            # Praat's octave cost: per octave of lag above LAG_MIN, taken off the local score
JUMP_COST = 0.35              # Praat's octave-jump cost: per octave between the lags of consecutive frames
CENTS_PER_NAT = 1200.0 / math.log(2.0)


# ------------------------------------------------------------------------------------------------ host tables (float64)
def hann_periodic(n: int = FRAME) -> np.ndarray:
    return packed.hann_periodic(n)


def lags() -> np.ndarray:
    """the lags of the lag basis rows: 0, then LAG_MIN..LAG_MAX"""
    return np.concatenate([[0], np.arange(LAG_MIN, LAG_MAX + 1)]).astype(np.int64)


def irfft_matrix(fft_size: int = FFT_SIZE) -> np.ndarray:
    """[fft_size, nb]: c = irfft(X) of a real spectrum X over the nb = fft_size/2 + 1 one-sided bins (np.fft.irfft)"""
    return onesided_dft(fft_size, inverse=True)[0]


def freqt_matrix(m1: int, m2: int, alpha: float) -> np.ndarray:
    """[m2 + 1, m1 + 1]: SPTK freqt (frequency warping of a cepstrum of order m1 to order m2) as the linear map it is: the
    published recursion run on every unit vector at once"""
    b = 1.0 - alpha * alpha
    eye = np.eye(m1 + 1)
    g = np.zeros((m2 + 1, m1 + 1))
    for i in range(m1, -1, -1):
        d = g.copy()
        g[0] = eye[i] + alpha * d[0]
        if m2 >= 1:
            g[1] = b * d[0] + alpha * d[1]
        for j in range(2, m2 + 1):
            g[j] = d[j - 1] + alpha * (d[j] - g[j - 1])
    return g


def sp2mc_matrix(order: int = ORDER, alpha: float = ALPHA, fft_size: int = FFT_SIZE) -> np.ndarray:
    """[order + 1, nb] float64: mc = S @ ln(P) is pysptk.sp2mc (irfft of the log power spectrum, c[0] / 2, freqt) on the
    nb one-sided bins.  freqt runs over the whole fft_size-point cepstrum, as pysptk does."""
    c = irfft_matrix(fft_size)
    c[0] *= 0.5
    return freqt_matrix(fft_size - 1, order, alpha) @ c


def lag_basis(fft_size: int = FFT_SIZE) -> np.ndarray:
    """[len(lags()), nb] float64: r(tau) = L @ P is the autocorrelation of the zero-padded frame at the lags (the inverse
    DFT of the power spectrum; no wrap-around while tau + FRAME <= fft_size)"""
    return onesided_dft(fft_size, rows=lags(), inverse=True)[0]


def window_gain() -> np.ndarray:
    """[len(lags())]: r_w(0) / r_w(tau) of the analysis window at the lags (entry 0: 1)"""
    w = hann_periodic()
    rw = np.array([np.dot(w[:FRAME - t], w[t:]) for t in lags()])
    return rw[0] / rw


def f0_tables():
    """(l2 [F0_STATES], oct [F0_STATES]) float64: log2 of the states' lags and the octave cost of each state"""
    l2 = np.log2(np.arange(LAG_MIN, LAG_MAX + 1, dtype=np.float64))
    return l2, OCTAVE_COST * (l2 - l2[0])


def frame_count(n: int) -> int:
    """frames of an n-sample signal: one per 5 ms, as Harvest produces"""
    return int(n) // HOP + 1


def mcd_from(cost, length):
    """10/ln10 * sqrt(2) * cost / length, float64; NaN where length == 0"""
    cost = np.asarray(cost, dtype=np.float64)
    length = np.asarray(length)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(length > 0, MCD_SCALE * cost / np.maximum(length, 1), np.nan)


def lf0_rmse_from(sse, length):
    """sqrt(sse / length) in nats, float64; NaN where length == 0"""
    sse = np.asarray(sse, dtype=np.float64)
    length = np.asarray(length)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(length > 0, np.sqrt(sse / np.maximum(length, 1)), np.nan)


def lf0_stats(lf0) -> tuple:
    """(mean, standard deviation) of the log-F0 values, float64 (the reference's logf0_statistics); NaN when empty"""
    lf0 = np.asarray(lf0, dtype=np.float64)
    return (float(lf0.mean()), float(lf0.std())) if lf0.size else (float("nan"), float("nan"))


# ------------------------------------------------------------------------------------------------------------ GPU passes
class MelCepstrum:
    """The feature pass on the GPU: waveforms -> per frame 24 mel-cepstral coefficients and a voicing flag; one launch per
    pass for a whole packed batch (framing, DFT contraction, log power, mcep and lag contractions, voicing + compaction).
    Tables are built once (float64 on the host, fp32 on the device)."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("MelCepstrum runs on the HIP path only (no CPU fallback)")
        self.nb, self.nbp = FFT_SIZE // 2 + 1, padded_bins(FFT_SIZE)
        self.n_mc, self.n_lag = pad4(ORDER + 1), pad4(len(lags()))          # 40, 208 rows (16-byte rows)
        mc = np.zeros((self.n_mc, self.nbp))
        mc[:ORDER + 1, :self.nb] = sp2mc_matrix()
        lg = np.zeros((self.n_lag, self.nbp))
        lg[:len(lags()), :self.nb] = lag_basis()
        gain = np.zeros(self.n_lag)
        gain[:len(lags())] = window_gain()
        f32 = lambda a: upload(a, self.device)
        self.window = f32(hann_periodic())
        self.dft = f32(dft_basis(FFT_SIZE, self.nbp)[:, :FRAME])                # [2 nbp, 512]: the padded half is zero
        self.mc_basis, self.lag_basis, self.gain = f32(mc), f32(lg), f32(gain)
        self._resampler = None
        self._f0_tables = None

    def f0_viterbi(self, r, voiced, segs, nseg: int, rows: int, out=None) -> dict:
        """the F0 tracker on the feature pass's own buffers, one launch: r [rows, 208] and voiced [rows]
        as dvae_voicing_compact read / wrote them, segs the device segment table -> lag [rows] int32, f0 [rows] fp32 (both
        0 on unvoiced frames), lf0v [rows] fp32: ln f0 of utterance s's voiced frames at rows row0 .. row0 + count[s], as
        feats.  out: buffers to write into (keys lag, f0, lf0v), for callers that own them."""
        if self._f0_tables is None:
            self._f0_tables = tuple(upload(t, self.device, np.float64) for t in f0_tables())
        l2, oct_ = self._f0_tables
        out = dict(out) if out is not None else dict(
            lag=torch.empty(rows, device=self.device, dtype=torch.int32),
            f0=torch.empty(rows, device=self.device, dtype=torch.float32),
            lf0v=torch.empty(rows, device=self.device, dtype=torch.float32))
        back = torch.empty((rows, F0_BACK_LD), device=self.device, dtype=torch.uint8)
        check(lib().dvae_f0_viterbi(ptr(r), self.n_lag, F0_STATES, ptr(self.gain), ptr(voiced), ptr(segs), nseg, ptr(l2),
                                    ptr(oct_), JUMP_COST, float(SAMPLE_RATE), LAG_MIN, ptr(back), ptr(out["lag"]),
                                    ptr(out["f0"]), ptr(out["lf0v"]), stream()), "dvae_f0_viterbi")
        return out

    def to16k(self, wavs: Sequence, srs: Sequence[int] = None) -> list:
        """1-D waveforms (numpy / tensors) at `srs` (default all 16 kHz) -> 1-D fp32 arrays / device tensors at 16 kHz
        (preprocess.resample_batch: one launch for those at other rates)"""
        wavs = [flat(w) for w in wavs]
        if srs is None:
            return wavs
        if len(srs) != len(wavs):
            raise ValueError("MelCepstrum: one sample rate per waveform")
        todo = [i for i, (w, sr) in enumerate(zip(wavs, srs)) if int(sr) != SAMPLE_RATE and w.shape[0] > 0]
        if todo:
            if self._resampler is None:
                self._resampler = Resampler(self.device)
            ys = resample_batch([wavs[i] for i in todo], [int(srs[i]) for i in todo], resampler=self._resampler)
            wavs = list(wavs)
            for i, y in zip(todo, ys):
                wavs[i] = y
        return wavs

    def packed(self, wavs: Sequence, srs: Sequence[int] = None, f0: bool = False) -> dict:
        """the whole feature pass on one packed batch, results left on the device:
          table   [nseg, 4] int64 numpy {row0, M, sample0, n}
          feats   [rows, 24] device: utterance s's voiced frames' coefficients at rows row0 .. row0 + count[s]
          count   [nseg] int64 numpy (one sync)
          mc      [rows, 40] device: every frame's coefficients (0..35; 36..39 zero)
          voiced  [rows] int32 device;  peak [rows] device: max r_n;  r [rows, 208] device: r(0), r(20..225)
        f0=True: one more launch (f0_viterbi) adds  lag [rows] int32, f0 [rows] (Hz, 0 unvoiced), lf0v [rows] (ln f0 of
        the voiced frames, at the rows of feats)"""
        L = lib()
        sigs = self.to16k(wavs, srs)
        if not sigs:
            raise ValueError("MelCepstrum: empty batch")
        ns = [int(s.shape[0]) for s in sigs]
        wav, offs = pack(sigs, self.device)
        ms = [frame_count(n) for n in ns]
        table = segment_table(ms, offs, ns)
        segs = upload(table, self.device, np.int64)
        rows, nseg = int(sum(ms)), len(ns)
        f = lambda *shape: torch.empty(shape, device=self.device, dtype=torch.float32)
        frames = f(rows, FRAME)
        check(L.dvae_stft_frames_seg(ptr(wav), ptr(segs), nseg, rows, ptr(self.window), ptr(frames), FRAME, HOP,
                                     FRAME // 2, stream()), "dvae_stft_frames_seg")
        reim = f(rows, 2 * self.nbp)
        pinned_gemm(frames, self.dft, reim, FRAME)
        del frames
        pw, lp = f(rows, self.nbp), f(rows, self.nbp)
        check(L.dvae_log_power(ptr(reim), ptr(pw), ptr(lp), rows, self.nb, self.nbp, POWER_FLOOR, stream()),
              "dvae_log_power")
        del reim
        mc, r = f(rows, self.n_mc), f(rows, self.n_lag)
        pinned_gemm(lp, self.mc_basis, mc, self.nbp)
        pinned_gemm(pw, self.lag_basis, r, self.nbp)
        del pw, lp
        feats, peak = f(rows, DIM), f(rows)
        voiced = torch.empty(rows, device=self.device, dtype=torch.int32)
        count = torch.empty(nseg, device=self.device, dtype=torch.int32)
        check(L.dvae_voicing_compact(ptr(r), self.n_lag, len(lags()) - 1, ptr(self.gain), ptr(mc), self.n_mc, ptr(segs),
                                     nseg, VOICED_PEAK, VOICED_REL_POWER, ptr(peak), ptr(voiced), ptr(feats), ptr(count),
                                     stream()), "dvae_voicing_compact")
        out = dict(table=table, feats=feats, count=None, mc=mc, voiced=voiced, peak=peak, r=r)
        if f0:
            out.update(self.f0_viterbi(r, voiced, segs, nseg, rows))
        out["count"] = count.cpu().numpy().astype(np.int64)
        return out

    def batch(self, wavs: Sequence, srs: Sequence[int] = None) -> list:
        """waveforms -> list of (mc [M, 24] float32 numpy, voiced [M] bool numpy), M = n // 80 + 1 frames"""
        out = self.packed(wavs, srs)
        mc, voiced = out["mc"].cpu().numpy(), out["voiced"].cpu().numpy().astype(bool)
        return [(mc[r0:r0 + m, :DIM].copy(), voiced[r0:r0 + m].copy()) for r0, m in out["table"][:, :2]]

    def f0_batch(self, wavs: Sequence, srs: Sequence[int] = None) -> list:
        """waveforms -> list of (f0 [M] float32 numpy in Hz, 0 on unvoiced frames; voiced [M] bool numpy)"""
        out = self.packed(wavs, srs, f0=True)
        f0, voiced = out["f0"].cpu().numpy(), out["voiced"].cpu().numpy().astype(bool)
        return [(f0[r0:r0 + m].copy(), voiced[r0:r0 + m].copy()) for r0, m in out["table"][:, :2]]


def check_pairs(nx, ny, names=None):
    """ValueError naming the first pair the DTW kernel does not support (min(N, M) > DTW_MAX_SHORT voiced frames)"""
    for p, (a, b) in enumerate(zip(nx, ny)):
        if a > 0 and b > 0 and min(a, b) > DTW_MAX_SHORT:
            who = names[p] if names is not None else f"pair {p}"
            raise ValueError(f"{who}: {a} x {b} voiced frames; the DTW kernel supports min(N, M) <= {DTW_MAX_SHORT} "
                             f"({DTW_MAX_SHORT * HOP / SAMPLE_RATE:.0f} s of voiced speech)")


def _dtw_launch(x, y, pairs, names=None, lf0x=None, lf0y=None):
    """pairs [P, 4] int64 numpy {x_row0, nx, y_row0, ny} into device buffers x, y [., 24] -> (cost, length) numpy; with
    lf0x, lf0y (fp32 device, one value per row of x, y) through dvae_dtw_batch_f0 -> (cost, length, sse)"""
    pairs = np.ascontiguousarray(pairs, dtype=np.int64)
    check_pairs(pairs[:, 1], pairs[:, 3], names)
    dev = x.device
    pd = upload(pairs, dev, np.int64)
    cost = torch.empty(len(pairs), device=dev, dtype=torch.float64)
    length = torch.empty(len(pairs), device=dev, dtype=torch.int64)
    if lf0x is None:
        check(lib().dvae_dtw_batch(ptr(x), ptr(y), ptr(pd), pairs.ctypes.data, len(pairs), ptr(cost), ptr(length),
                                   stream()), "dvae_dtw_batch")
        return cost.cpu().numpy(), length.cpu().numpy()
    sse = torch.empty(len(pairs), device=dev, dtype=torch.float64)
    check(lib().dvae_dtw_batch_f0(ptr(x), ptr(y), ptr(lf0x), ptr(lf0y), ptr(pd), pairs.ctypes.data, len(pairs), ptr(cost),
                                  ptr(length), ptr(sse), stream()), "dvae_dtw_batch_f0")
    return cost.cpu().numpy(), length.cpu().numpy(), sse.cpu().numpy()


def dtw_batch(xs: Sequence, ys: Sequence, device="cuda"):
    """exact DTW of every pair (xs[p] [N_p, 24], ys[p] [M_p, 24]) in one launch -> (cost float64 [P], length int64 [P]);
    cost NaN and length 0 where a side is empty"""
    if len(xs) != len(ys) or not xs:
        raise ValueError("dtw_batch: one y per x, at least one pair")
    x, xr, nx = pack_rows([np.asarray(s, dtype=np.float32).reshape(-1, DIM) for s in xs], DIM, device)
    y, yr, ny = pack_rows([np.asarray(s, dtype=np.float32).reshape(-1, DIM) for s in ys], DIM, device)
    pairs = np.stack([xr, nx, yr, ny], axis=1).astype(np.int64)
    return _dtw_launch(x, y, pairs)


def dtw_batch_f0(xs: Sequence, ys: Sequence, lf0xs: Sequence, lf0ys: Sequence, device="cuda"):
    """dtw_batch that also carries the squared log-F0 difference along each pair's path (lf0xs[p] [N_p], lf0ys[p] [M_p])
    -> (cost float64 [P], length int64 [P], sse float64 [P]); cost and length are dtw_batch's bits"""
    if not (len(xs) == len(ys) == len(lf0xs) == len(lf0ys)) or not xs:
        raise ValueError("dtw_batch_f0: one y, lf0x and lf0y per x, at least one pair")
    x, xr, nx = pack_rows([np.asarray(s, dtype=np.float32).reshape(-1, DIM) for s in xs], DIM, device)
    y, yr, ny = pack_rows([np.asarray(s, dtype=np.float32).reshape(-1, DIM) for s in ys], DIM, device)
    lx, lxr, lnx = pack_rows([np.asarray(s, dtype=np.float32).reshape(-1, 1) for s in lf0xs], 1, device)
    ly, lyr, lny = pack_rows([np.asarray(s, dtype=np.float32).reshape(-1, 1) for s in lf0ys], 1, device)
    if not (np.array_equal(xr, lxr) and np.array_equal(nx, lnx) and np.array_equal(yr, lyr) and np.array_equal(ny, lny)):
        raise ValueError("dtw_batch_f0: one log-F0 value per feature row")
    pairs = np.stack([xr, nx, yr, ny], axis=1).astype(np.int64)
    return _dtw_launch(x, y, pairs, lf0x=lx, lf0y=ly)


def mcd_batch(converted_wavs: Sequence, reference_wavs: Sequence, converted_srs=None, reference_srs=None, names=None,
              features: MelCepstrum = None, f0: bool = False) -> dict:
    """MCD of every (converted, reference) pair; both sides go through ONE feature pass and the pairs through one DTW
    launch.  -> dict of numpy arrays over the pairs: mcd (dB, NaN where a side has no voiced frames), cost, path_length,
    frames_converted / frames_reference, voiced_converted / voiced_reference; and mean_mcd over the finite ones (NaN if
    none).  names: per pair, for the error that names a pair too long for the DTW kernel.
    f0=True: the feature pass also tracks F0, the DTW launch is dvae_dtw_batch_f0 (mcd, cost, path_length
    unchanged to the bit) and the dict gains lf0_rmse (nats) and lf0_rmse_cents along the MCD's path (NaN where mcd is),
    lf0_mean_converted / lf0_std_converted / lf0_mean_reference / lf0_std_reference (ln Hz over each utterance's voiced
    frames, NaN without any), mean_lf0_rmse_cents over the finite ones, and the pooled lf0_pooled_mean_converted /
    lf0_pooled_std_converted / lf0_pooled_mean_reference / lf0_pooled_std_reference over all voiced frames of a side."""
    P = len(converted_wavs)
    if P != len(reference_wavs) or P == 0:
        raise ValueError("mcd_batch: one reference per converted waveform, at least one pair")
    fe = features or MelCepstrum()
    srs = None
    if converted_srs is not None or reference_srs is not None:
        srs = [int(s) for s in (converted_srs if converted_srs is not None else [SAMPLE_RATE] * P)] + \
              [int(s) for s in (reference_srs if reference_srs is not None else [SAMPLE_RATE] * P)]
    out = fe.packed(list(converted_wavs) + list(reference_wavs), srs, f0=f0)
    table, count = out["table"], out["count"]
    pairs = np.stack([table[:P, 0], count[:P], table[P:, 0], count[P:]], axis=1)
    if f0:
        cost, length, sse = _dtw_launch(out["feats"], out["feats"], pairs, names, lf0x=out["lf0v"], lf0y=out["lf0v"])
    else:
        cost, length = _dtw_launch(out["feats"], out["feats"], pairs, names)
    mcd = mcd_from(cost, length)
    fin = mcd[np.isfinite(mcd)]
    res = dict(mcd=mcd, cost=cost, path_length=length, frames_converted=table[:P, 1].copy(),
               frames_reference=table[P:, 1].copy(), voiced_converted=count[:P].copy(), voiced_reference=count[P:].copy(),
               mean_mcd=float(fin.mean()) if fin.size else float("nan"))
    if f0:
        rmse = lf0_rmse_from(sse, length)
        lf0v = out["lf0v"].cpu().numpy()
        per = [lf0v[r0:r0 + k] for r0, k in zip(table[:, 0], count)]      # ln f0 of each utterance's voiced frames
        stats = np.array([lf0_stats(v) for v in per], dtype=np.float64).reshape(2 * P, 2)
        fin = rmse[np.isfinite(rmse)]
        res.update(lf0_rmse=rmse, lf0_rmse_cents=CENTS_PER_NAT * rmse,
                   lf0_mean_converted=stats[:P, 0].copy(), lf0_std_converted=stats[:P, 1].copy(),
                   lf0_mean_reference=stats[P:, 0].copy(), lf0_std_reference=stats[P:, 1].copy(),
                   mean_lf0_rmse_cents=float(CENTS_PER_NAT * fin.mean()) if fin.size else float("nan"))
        for side, sl in (("converted", slice(0, P)), ("reference", slice(P, 2 * P))):
            m, sd = lf0_stats(np.concatenate(per[sl]))
            res[f"lf0_pooled_mean_{side}"], res[f"lf0_pooled_std_{side}"] = m, sd
    return res


# ------------------------------------------------------------------------------------------------------------------ CLI
def utterance_id(path) -> str:
    """the last `_` token of the stem: `convert_<src>_to_<trg>_<utt>.wav` and VCTK's `p226_<utt>.wav` both give <utt>"""
    return Path(path).stem.rsplit("_", 1)[-1]


def pair_files(converted: Sequence, reference: Sequence):
    """-> (pairs [(utt, converted path, reference path)] in sorted utterance order, unmatched converted paths, unmatched
    reference paths).  A second file with the same utterance id on one side is unmatched."""
    def index(paths):
        by, extra = {}, []
        for p in sorted(paths, key=lambda q: str(q)):
            u = utterance_id(p)
            if u in by:
                extra.append(p)
            else:
                by[u] = p
        return by, extra

    cv, cv_extra = index(converted)
    rf, rf_extra = index(reference)
    pairs = [(u, cv[u], rf[u]) for u in sorted(cv) if u in rf]
    un_c = sorted([cv[u] for u in cv if u not in rf] + cv_extra, key=lambda q: str(q))
    un_r = sorted([rf[u] for u in rf if u not in cv] + rf_extra, key=lambda q: str(q))
    return pairs, un_c, un_r


def _parse(argv):
    p = argparse.ArgumentParser(prog="python -m dvae_amd.evaluate",
                                description="Mel-cepstral distortion of converted .wav files against reference .wav files "
                                            "(the reference's preprocessing/MCD_calculate.py), on the GPU.")
    p.add_argument("converted_dir", type=Path, help="directory of converted *.wav (e.g. <run>/generation/<src>_to_<trg>)")
    p.add_argument("reference_dir", type=Path, help="directory of ground-truth *.wav (e.g. <wav16>/<trg>)")
    p.add_argument("--json", type=Path, default=None, help="where to write the results (default <converted_dir>/mcd.json)")
    p.add_argument("--f0", action="store_true",
                   help="also track F0 and report the log-F0 RMSE (cents) along each pair's MCD alignment, with the "
                        "per-file and pooled log-F0 mean and standard deviation")
    return p.parse_args(argv)


def main(argv=None) -> int:
    args = _parse(sys.argv[1:] if argv is None else argv)
    for d in (args.converted_dir, args.reference_dir):
        if not d.is_dir():
            print(f"evaluate: {d} is not a directory", file=sys.stderr)
            return 2
    pairs, un_c, un_r = pair_files(sorted(args.converted_dir.glob("*.wav")), sorted(args.reference_dir.glob("*.wav")))
    result = dict(converted_dir=str(args.converted_dir), reference_dir=str(args.reference_dir), pairs=[],
                  mean_mcd=None, scored=0, no_voiced=[],
                  unmatched=dict(converted=[str(p) for p in un_c], reference=[str(p) for p in un_r]))
    out_path = args.json or args.converted_dir.joinpath("mcd.json")
    if not pairs:
        print(f"evaluate: no converted file in {args.converted_dir} matches a reference file in {args.reference_dir} "
              "by utterance id (the last '_' token of the file name)", file=sys.stderr)
        out_path.write_text(json.dumps(result, indent=1) + "\n")
        return 1
    cw, cs, rw, rs = [], [], [], []
    for _, c, r in pairs:
        w, sr = read_wav(c)
        cw.append(w)
        cs.append(sr)
        w, sr = read_wav(r)
        rw.append(w)
        rs.append(sr)
    res = mcd_batch(cw, rw, cs, rs, names=[f"{c.name} / {r.name}" for _, c, r in pairs], f0=args.f0)
    for p, (u, c, r) in enumerate(pairs):
        m = float(res["mcd"][p])
        row = dict(utterance=u, converted=str(c), reference=str(r), mcd=m if math.isfinite(m) else None,
                   path_length=int(res["path_length"][p]), frames_converted=int(res["frames_converted"][p]),
                   frames_reference=int(res["frames_reference"][p]), voiced_converted=int(res["voiced_converted"][p]),
                   voiced_reference=int(res["voiced_reference"][p]))
        result["pairs"].append(row)
        if math.isfinite(m):
            print(f"utterance {u} mcd: {m}")
        else:
            sides = [s for s, k in (("converted", "voiced_converted"), ("reference", "voiced_reference")) if row[k] == 0]
            result["no_voiced"].append(u)
            print(f"utterance {u} mcd: nan (no voiced frames in the {' and '.join(sides)} file)")
    scored = [r["mcd"] for r in result["pairs"] if r["mcd"] is not None]
    result["scored"] = len(scored)
    result["mean_mcd"] = res["mean_mcd"] if scored else None
    if args.f0:
        num = lambda v: float(v) if math.isfinite(float(v)) else None
        hz = lambda m: f"{math.exp(m)} Hz" if math.isfinite(m) else "nan"
        for p, row in enumerate(result["pairs"]):
            row.update(lf0_rmse=num(res["lf0_rmse"][p]), lf0_rmse_cents=num(res["lf0_rmse_cents"][p]),
                       **{f"lf0_{k}_{side}": num(res[f"lf0_{k}_{side}"][p]) for k in ("mean", "std")
                          for side in ("converted", "reference")})
            print(f"utterance {row['utterance']} lf0 rmse: {float(res['lf0_rmse_cents'][p])} cents (converted mean "
                  f"{hz(float(res['lf0_mean_converted'][p]))}, reference mean {hz(float(res['lf0_mean_reference'][p]))})")
        result["mean_lf0_rmse_cents"] = num(res["mean_lf0_rmse_cents"])
        for k in ("lf0_pooled_mean_converted", "lf0_pooled_std_converted", "lf0_pooled_mean_reference",
                  "lf0_pooled_std_reference"):
            result[k] = num(res[k])
        print(f"mean lf0 rmse: {res['mean_lf0_rmse_cents']} cents over {len(scored)} of {len(pairs)} pairs; pooled log-F0 "
              f"mean / std: converted {res['lf0_pooled_mean_converted']} / {res['lf0_pooled_std_converted']}, reference "
              f"{res['lf0_pooled_mean_reference']} / {res['lf0_pooled_std_reference']}")
    print(f"mean mcd: {res['mean_mcd']} over {len(scored)} of {len(pairs)} pairs"
          + (f"; unmatched: {len(un_c)} converted, {len(un_r)} reference" if un_c or un_r else ""))
    out_path.write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
