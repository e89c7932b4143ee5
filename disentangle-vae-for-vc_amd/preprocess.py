"""Corpus preprocessing on the GPU: a VCTK `.wav` tree -> the mel corpus `<out>/<speaker>/*_mel.npy` that
`SpeechDatasetGVAE` / `GpuPairLoader` read.  The reference's `preprocessing.sh` step:

    python -m dvae_amd.preprocess <datasets_root> [-o OUT] [-d VCTK] [-s] (--no_trim | --trim) [--batch-seconds S] [--workers W]

mirrors the reference's preprocessing/dataset_preprocess.py -> encoder/preprocess.py:78-138,153-170 -> encoder/audio.py:22-51
`preprocess_wav`:

    librosa.load(path, sr=None, duration=600)           read_wav (numpy RIFF reader; float32 mono, first 600 s)
    librosa.resample(wav, sr, 16000)                     resampy kaiser_best (fix=True: ceil(n * 16000 / sr) samples)
    normalize_volume(wav, -30, increase_only=True)       float64 mean square, gain only where it is > 1
    trim_long_silences(wav)            (--trim only)     window energies, per-utterance threshold, the reference's smoothing
    wav_to_mel_spectrogram -> np.save([80, M])           MelFrontend, pinned: one k-split, segmented passes

One launch per pass for a whole batch of utterances (any source rates and lengths, packed back to back), all on one stream;
host threads decode a bounded window ahead and a separate pool writes, overlapped with the GPU passes (preprocess_vctk).  An output's bits depend only on its own file: not on the batch it lands in, on
--batch-seconds, on --workers or on timing.

resampy and librosa are not dependencies: the kaiser_best filter is restated from resampy's published construction
(`sinc_window(64, 9, kaiser(14.769656459379492), rolloff=0.9475937167399596)`, resampy/interp.py `resample_f`) and its
parity with the real package is UNPINNED.  Differences from the reference, on purpose: the corpus is
float32 (the reference wrote float64 from lws; float32 carries every bit computed here); a silent file is skipped and
reported (the reference wrote a NaN mel); webrtcvad is absent, so without a flag the tool stops as the reference does when
webrtcvad does not import: --no_trim builds the corpus untrimmed, --trim trims with the energy detector of vad_packed below
(this project's own; its parity with webrtcvad is UNPINNED).  Kept on purpose: the reference's `len(frames) < partials_n_frames` test never
fires (`frames` is [80, M], len 80), so every decodable utterance is written however short.
"""
from __future__ import annotations

import argparse
import math
import struct
import sys
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Sequence

import numpy as np
import torch

from ._lib import check, lib, ptr, stream
from .frontend import MelFrontend
from .packed import flat, pack, pad4, upload  # noqa: F401  (pack: its callers import it from here too)

SAMPLE_RATE = 16000
RESAMPLE_TILE = 256           # DVAE_RESAMPLE_TILE
VOLUME_TILE = 2048            # DVAE_VOLUME_TILE
KAISER_BEST = dict(num_zeros=64, precision=9, beta=14.769656459379492, rolloff=0.9475937167399596)
VAD_WINDOW = 480              # DVAE_VAD_WINDOW: 30 ms at 16 kHz (audio.py vad_window_length)
VAD_MA_WIDTH = 8              # DVAE_VAD_MA_WIDTH (vad_moving_average_width)
VAD_MAX_SILENCE = 6           # DVAE_VAD_MAX_SILENCE (vad_max_silence_length)
VAD_PREEMPH = 0.97            # DVAE_VAD_PREEMPH
VAD_BINS, VAD_BIN_OFFSET = 96, 80                                 # b = clamp(ilogb(E) + 80, 0, 95)
VAD_BIN_FLOOR, VAD_BIN_ABOVE_P10, VAD_BIN_BELOW_P90 = 66, 3, 5    # t = max(66, min(b10 + 3, b90 - 5))
TOO_SHORT_TO_TRIM = "shorter than one 30 ms window"
NO_SPEECH = "no speech detected"
DATASETS = ("VCTK",)
NO_TRIM_MESSAGE = ("Package 'webrtcvad' not found. This package enables noise removal and is recommended. Please install "
                   "and try again. If installation fails, use --no_trim to disable this error message.")


# ------------------------------------------------------------------------------------------------------------ wav reader
_PCM, _FLOAT, _EXTENSIBLE = 1, 3, 0xFFFE


def read_wav(path, duration: float = 600.0):
    """RIFF/WAVE file -> (float32 mono [n], sample rate), the first round(sr * duration) frames (librosa.load(path,
    sr=None, duration=...) through soundfile): PCM u8 / s16 / s24 / s32, IEEE float32 / float64, WAVE_FORMAT_EXTENSIBLE
    with those subtypes; scaled as soundfile does ((u8 - 128) / 2^7, s16 / 2^15, s24 / 2^23, s32 / 2^31); mono = the
    float32 mean over channels.  Unknown chunks (LIST, fact, ...) and their odd-size pad bytes are skipped.  Anything
    else raises ValueError naming the file."""
    path = str(path)
    with open(path, "rb") as f:
        raw = f.read()

    def bad(why):
        return ValueError(f"{path}: {why}")

    if len(raw) < 12 or raw[:4] != b"RIFF" or raw[8:12] != b"WAVE":
        raise bad("not a RIFF/WAVE file")
    fmt, data, pos = None, None, 12
    while pos + 8 <= len(raw):
        cid, size = raw[pos:pos + 4], struct.unpack_from("<I", raw, pos + 4)[0]
        body = pos + 8
        if cid == b"fmt ":
            if size < 16 or body + size > len(raw):
                raise bad("truncated fmt chunk")
            tag, ch, sr, _, align, bits = struct.unpack_from("<HHIIHH", raw, body)
            if tag == _EXTENSIBLE:
                if size < 40:
                    raise bad("truncated WAVE_FORMAT_EXTENSIBLE fmt chunk")
                tag = struct.unpack_from("<H", raw, body + 24)[0]      # first two bytes of the SubFormat GUID
            fmt = (tag, ch, sr, align, bits)
        elif cid == b"data":
            if fmt is None:
                raise bad("data chunk before fmt chunk")
            if body + size > len(raw):
                raise bad(f"truncated data chunk ({len(raw) - body} of {size} bytes)")
            data = raw[body:body + size]
            break
        pos = body + size + (size & 1)
    if fmt is None or data is None:
        raise bad("no fmt or data chunk")
    tag, ch, sr, align, bits = fmt
    if ch < 1 or sr < 1:
        raise bad(f"{ch} channels at {sr} Hz")
    width = bits // 8
    if bits % 8 or align != width * ch:
        raise bad(f"unsupported sample layout ({bits} bits, block align {align})")
    if tag == _PCM and bits in (8, 16, 24, 32):
        pass
    elif tag == _FLOAT and bits in (32, 64):
        pass
    else:
        raise bad(f"unsupported WAVE format {tag:#x} with {bits} bits (PCM 8/16/24/32 and IEEE float 32/64 only)")
    n = len(data) // align
    if duration is not None:
        n = min(n, int(round(sr * duration)))
    buf = np.frombuffer(data, dtype=np.uint8, count=n * align)
    if tag == _FLOAT:
        x = buf.view("<f4" if bits == 32 else "<f8").astype(np.float32)
    elif bits == 8:
        x = ((buf.astype(np.float32) - 128.0) / 128.0).astype(np.float32)
    elif bits == 16:
        x = (buf.view("<i2").astype(np.float64) / 2.0 ** 15).astype(np.float32)
    elif bits == 24:
        b = buf.reshape(-1, 3).astype(np.int32)
        v = (b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)).astype(np.int32)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = (v.astype(np.float64) / 2.0 ** 23).astype(np.float32)
    else:
        x = (buf.view("<i4").astype(np.float64) / 2.0 ** 31).astype(np.float32)
    x = x.reshape(n, ch)
    wav = x[:, 0].copy() if ch == 1 else x.mean(axis=1, dtype=np.float32)
    return np.ascontiguousarray(wav, dtype=np.float32), int(sr)


# --------------------------------------------------------------------------------------------------- resampy kaiser_best
def kaiser_best_window():
    """resampy.filters.sinc_window(num_zeros=64, precision=9, window=kaiser(beta), rolloff) -> (win [32769] float64,
    num_table 512, rolloff)"""
    nz, prec, beta, rolloff = (KAISER_BEST[k] for k in ("num_zeros", "precision", "beta", "rolloff"))
    num_table = 2 ** prec
    n = num_table * nz
    sinc = rolloff * np.sinc(rolloff * np.linspace(0, nz, num=n + 1, endpoint=True))
    taper = np.kaiser(2 * n + 1, beta)[n:]
    return taper * sinc, num_table, rolloff


def resample_lengths(n: int, sr_old: int, sr_new: int = SAMPLE_RATE):
    """-> (n_valid, n_out): resampy's int(n * ratio) outputs of the filter, librosa's fix=True length ceil(n * ratio)"""
    g = math.gcd(sr_old, sr_new)
    P, Q = sr_new // g, sr_old // g
    n_valid = n * P // Q
    if n_valid != int(n * (float(sr_new) / sr_old)):          # resampy rounds in float64; never silently differ
        raise ValueError(f"resample: int({n} * {sr_new}/{sr_old}) differs from the exact floor")
    return n_valid, -(-n * P // Q)


def resample_filter(sr_old: int, sr_new: int = SAMPLE_RATE) -> dict:
    """Host tables of resampy.resample(x, sr_old, sr_new, filter='kaiser_best') (float64):
      P, Q          ratio = sr_new / sr_old = P / Q in lowest terms; output t reads around input m = floor(t Q / P) at
                    phase t Q - m P (the period of the filter offsets is P outputs)
      scale         min(1, ratio);  index_step  int(scale * 512) (the truncation is resampy's)
      win, delta    the interpolation table (scaled by ratio when downsampling) and its forward difference
      weights       [P, taps] float64: phase p's taps in input order, tap c reads x[m - base + c] (zero where resampy's
                    left / right wings end, so that every phase has `taps` of them)
      base, taps"""
    if sr_old < 1 or sr_new < 1:
        raise ValueError("resample_filter: sample rates must be positive")
    g = math.gcd(sr_old, sr_new)
    P, Q = sr_new // g, sr_old // g
    ratio = float(sr_new) / sr_old
    scale = min(1.0, ratio)
    win, num_table, _ = kaiser_best_window()
    if ratio < 1:
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    nwin = win.shape[0]
    index_step = int(scale * num_table)
    # frac * num_table of phase p, exactly: num / den with frac = scale * p / P
    sn, sd = (P, Q) if ratio < 1 else (1, 1)
    den = sd * P

    def wing(p):
        num = num_table * sn * p
        off, eta = num // den, (num % den) / den
        cnt = (nwin - off) // index_step
        idx = off + index_step * np.arange(cnt)
        return win[idx] + eta * delta[idx]

    lefts = [wing(p) for p in range(P)]
    rights = [wing(P - p) for p in range(P)]           # frac' = scale - frac
    base = max(len(l) for l in lefts) - 1
    taps = base + 1 + max(len(r) for r in rights)
    w = np.zeros((P, taps), dtype=np.float64)
    for p in range(P):
        l, r = lefts[p], rights[p]
        w[p, base - np.arange(len(l))] = l
        w[p, base + 1:base + 1 + len(r)] = r
    return dict(P=P, Q=Q, ratio=ratio, scale=scale, index_step=index_step, num_table=num_table, win=win, delta=delta,
                weights=w, base=base, taps=taps)


# ------------------------------------------------------------------------------------------------------------ GPU passes
class Resampler:
    """Packed-batch resampler to `sr_new` on the GPU (dvae_resample_batch): one launch for utterances of any source rates
    and lengths.  The per-phase float64 weights of each source rate are rounded to fp32 once and kept on the device."""

    def __init__(self, device="cuda", sr_new: int = SAMPLE_RATE):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("Resampler runs on the HIP path only (no CPU fallback)")
        self.sr_new = int(sr_new)
        self._ids, self._rows, self._chunks, self._lds = {}, [], [], []
        self._weights = None

    def _filter(self, sr_old: int) -> int:
        sr_old = int(sr_old)
        if sr_old not in self._ids:
            if sr_old == self.sr_new:                  # the identity inside a packed batch: y = fmaf(1, x, 0) = x
                P, Q, base, taps, w = 1, 1, 0, 1, np.ones(1, dtype=np.float32)
            else:
                t = resample_filter(sr_old, self.sr_new)
                P, Q, base, taps, w = t["P"], t["Q"], t["base"], t["taps"], t["weights"].astype(np.float32).ravel()
            lds = lib().dvae_resample_lds_floats(P, Q, taps)
            if lds < 0:
                raise ValueError(f"Resampler: {sr_old} -> {self.sr_new} Hz needs more LDS than a workgroup has")
            woff = sum(c.size for c in self._chunks)
            self._rows.append([P, Q, taps, base, woff, 0])
            self._chunks.append(w)
            self._lds.append(lds)
            self._ids[sr_old] = len(self._rows) - 1
            self._weights = None
        return self._ids[sr_old]

    def _tables(self):
        if self._weights is None:
            self._weights = upload(np.concatenate(self._chunks), self.device)
            self._filters = upload(self._rows, self.device, np.int64)
        return self._weights, self._filters

    def plan(self, lengths: Sequence[int], srs: Sequence[int], tile=RESAMPLE_TILE):
        """-> (table [nseg, 6] int64 {in0, n_in, out0, n_out, n_valid, filter}, tiles [ntiles, 2] int64, filter ids);
        ValueError when an utterance is too short for resampy (int(n * ratio) < 1)"""
        for n, sr in zip(lengths, srs):
            if n < 1 or (sr != self.sr_new and resample_lengths(n, sr, self.sr_new)[0] < 1):
                raise ValueError(f"resample: {n} samples at {sr} Hz is too short to resample to {self.sr_new} Hz")
        fid = np.asarray([self._filter(s) for s in srs], dtype=np.int32)
        n_in = np.asarray(lengths, dtype=np.int64)
        rows = np.asarray(self._rows, dtype=np.int64)
        table = np.zeros((len(n_in), 6), dtype=np.int64)
        nt = lib().dvae_resample_segment_table(n_in.ctypes.data, fid.ctypes.data, len(n_in), rows.ctypes.data, len(rows),
                                               tile, table.ctypes.data, None, 0)
        check(min(nt, 0), "dvae_resample_segment_table")
        tiles = np.zeros((nt, 2), dtype=np.int64)
        check(min(0, lib().dvae_resample_segment_table(n_in.ctypes.data, fid.ctypes.data, len(n_in), rows.ctypes.data,
                                                       len(rows), tile, table.ctypes.data, tiles.ctypes.data, nt)),
              "dvae_resample_segment_table")
        return table, tiles, fid

    def prepare(self, lengths: Sequence[int], srs: Sequence[int]) -> dict:
        """the host side of a launch: plan(), the tables on the device, the LDS size, the output length"""
        table, tiles, fid = self.plan(lengths, srs)
        self._tables()
        segs_d, tiles_d = (upload(a, self.device, np.int64) for a in (table, tiles))
        return dict(table=table, ntiles=len(tiles), segs=segs_d, tiles=tiles_d,
                    lds=max(self._lds[i] for i in set(fid.tolist())),
                    n_out=int(table[-1, 2] + pad4(table[-1, 3])))

    def launch(self, x, prep: dict, y=None):
        """dvae_resample_batch alone on prepared tables (prep holds them on the device until it is dropped)"""
        weights, filters = self._tables()
        if y is None:
            y = torch.empty(prep["n_out"], device=self.device, dtype=torch.float32)
        check(lib().dvae_resample_batch(ptr(x), ptr(y), ptr(prep["segs"]), ptr(filters), ptr(weights), ptr(prep["tiles"]),
                                        prep["ntiles"], prep["lds"], stream()), "dvae_resample_batch")
        return y

    def packed(self, x, lengths: Sequence[int], srs: Sequence[int]):
        """x: device fp32 packed as plan()'s in0 / n_in say -> (y device fp32 packed as out0 / n_out, table)"""
        prep = self.prepare(lengths, srs)
        return self.launch(x, prep), prep["table"]

    def __call__(self, wavs: Sequence, srs: Sequence[int]) -> list:
        return resample_batch(wavs, srs, self.sr_new, resampler=self)


def resample_batch(wavs: Sequence, srs: Sequence[int], sr_new: int = SAMPLE_RATE, resampler: Resampler = None,
                   device="cuda") -> list:
    """librosa.resample(wav, sr, sr_new) (resampy kaiser_best, fix=True) of every utterance, one launch for all: list of
    1-D device fp32 tensors of ceil(n * sr_new / sr) samples.  An utterance already at sr_new is returned unchanged (moved
    to the device, no launch)."""
    r = resampler or Resampler(device, sr_new)
    if len(wavs) != len(srs):
        raise ValueError("resample_batch: one rate per waveform")
    out = [None] * len(wavs)
    todo = []
    for i, (w, sr) in enumerate(zip(wavs, srs)):
        if int(sr) == r.sr_new:
            out[i] = torch.as_tensor(w).to(r.device, torch.float32).view(-1)
        else:
            todo.append(i)
    if todo:
        arrs = [flat(wavs[i]) for i in todo]
        x, _ = pack(arrs, r.device)
        y, table = r.packed(x, [a.shape[0] for a in arrs], [int(srs[i]) for i in todo])
        for j, i in enumerate(todo):
            out[i] = y[int(table[j, 2]):int(table[j, 2] + table[j, 3])]
    return out


def volume_prepare(table, device) -> dict:
    """the host side of dvae_volume_normalize: the DVAE_VOLUME_TILE tile map of `table`'s segments, on the device"""
    nseg = len(table)
    ntile = -(-table[:, 3] // VOLUME_TILE)
    tile_first = np.concatenate([[0], np.cumsum(ntile)]).astype(np.int64)
    tiles = np.zeros((int(tile_first[-1]), 2), dtype=np.int64)
    for s in range(nseg):
        a, b = tile_first[s], tile_first[s + 1]
        tiles[a:b, 0] = s
        tiles[a:b, 1] = np.arange(b - a, dtype=np.int64) * VOLUME_TILE
    to = lambda a: upload(a, device, np.int64)
    return dict(nseg=nseg, ntiles=len(tiles), segs=to(table), tiles=to(tiles), first=to(tile_first),
                part=torch.empty(len(tiles), device=device, dtype=torch.float64),
                ms=torch.empty(nseg, device=device, dtype=torch.float64),
                gain=torch.empty(nseg, device=device, dtype=torch.float32),
                silent=torch.empty(nseg, device=device, dtype=torch.int32))


def volume_launch(y, prep: dict, target_dbfs=-30.0, increase_only=True):
    """dvae_volume_normalize alone (three launches, no sync); results stay in prep["ms" | "gain" | "silent"]"""
    check(lib().dvae_volume_normalize(ptr(y), ptr(prep["segs"]), prep["nseg"], ptr(prep["tiles"]), prep["ntiles"],
                                      ptr(prep["first"]), ptr(prep["part"]), float(target_dbfs), int(bool(increase_only)),
                                      ptr(prep["ms"]), ptr(prep["gain"]), ptr(prep["silent"]), stream()),
          "dvae_volume_normalize")


def volume_packed(y, table, target_dbfs=-30.0, increase_only=True):
    """normalize_volume (audio.py:121-127) in place on the packed segments of `table` ({.., out0, n_out, ..} columns 2, 3)
    -> (mean square float64 [nseg] numpy, gain fp32 [nseg] numpy, silent bool [nseg] numpy); one sync at the end"""
    prep = volume_prepare(table, y.device)
    volume_launch(y, prep, target_dbfs, increase_only)
    return prep["ms"].cpu().numpy(), prep["gain"].cpu().numpy(), prep["silent"].cpu().numpy().astype(bool)


def normalize_volume_batch(wavs: Sequence, target_dbfs=-30.0, increase_only=True, device="cuda"):
    """normalize_volume(wav, target_dbfs, increase_only) of every utterance, one pass for all -> (list of 1-D device fp32
    tensors, silent mask [n] bool numpy).  A silent (all-zero) utterance comes back unchanged and flagged."""
    arrs = [flat(w) for w in wavs]
    if not arrs or any(a.shape[0] < 1 for a in arrs):
        raise ValueError("normalize_volume_batch: empty waveform")
    y, offs = pack(arrs, device)
    table = np.zeros((len(arrs), 6), dtype=np.int64)
    table[:, 2] = offs
    table[:, 3] = [a.shape[0] for a in arrs]
    _, _, silent = volume_packed(y, table, target_dbfs, increase_only)
    return [y[int(o):int(o + n)] for o, n in zip(table[:, 2], table[:, 3])], silent


def vad_prepare(table, device) -> dict:
    """the host side of dvae_vad_trim: the window map {segment, w} of `table`'s segments and each segment's first window in
    it, on the device, with the per-window and per-segment outputs"""
    table = np.ascontiguousarray(table, dtype=np.int64)
    nseg = len(table)
    W = table[:, 3] // VAD_WINDOW
    first = np.concatenate([[0], np.cumsum(W)]).astype(np.int64)
    nwin = int(first[-1])
    wins = np.zeros((nwin, 2), dtype=np.int64)
    wins[:, 0] = np.repeat(np.arange(nseg, dtype=np.int64), W)
    wins[:, 1] = np.arange(nwin, dtype=np.int64) - np.repeat(first[:-1], W)
    to = lambda a: upload(a, device, np.int64)
    i32 = lambda n: torch.empty(max(1, n), device=device, dtype=torch.int32)
    return dict(nseg=nseg, nwin=nwin, W=W, first=first, table=table, segs=to(table), wins=to(wins), win_first=to(first),
                E=torch.empty(max(1, nwin), device=device, dtype=torch.float64), bins=i32(nwin), flags=i32(nwin),
                keep=i32(nwin), dst=i32(nwin), t=i32(nseg), K=i32(nseg))


def vad_launch(y, prep: dict, out, want=()):
    """dvae_vad_trim alone (three launches, no sync): the kept windows of y's segments back to back in `out`, at the
    segments' own offsets; results stay in prep["K" | "keep" | "dst" | "bins"] and, where `want` names them, in
    prep["E" | "flags" | "t"]"""
    opt = lambda k: ptr(prep[k]) if k in want else None
    check(lib().dvae_vad_trim(ptr(y), ptr(out), prep["table"].ctypes.data, ptr(prep["segs"]), prep["nseg"],
                              ptr(prep["wins"]), prep["nwin"], ptr(prep["win_first"]), opt("E"), ptr(prep["bins"]),
                              opt("flags"), ptr(prep["keep"]), ptr(prep["dst"]), opt("t"), ptr(prep["K"]), stream()),
          "dvae_vad_trim")


def vad_packed(y, table, want=()):
    """trim_long_silences (audio.py:78-118) on the packed segments of `table` ({.., out0, n_out, ..} columns 2, 3), after
    volume normalisation, with the energy detector of include/dvae_hip.h ("silence trimming") in webrtcvad's place ->
    (out: a second device buffer with segment s's 480 K[s] kept samples at out0[s], the rest of it unwritten;
     K [nseg] numpy: the one device-to-host copy and sync;
     extras: `first` ([nseg + 1] numpy, segment s owns windows first[s] .. first[s + 1]) and the device tensors that `want`
     names of "E" (float64), "flags", "keep" (int32) per window and "t" (int32) per segment)"""
    bad = set(want) - {"E", "flags", "keep", "t"}
    if bad:
        raise ValueError(f"vad_packed: unknown outputs {sorted(bad)}")
    prep = vad_prepare(table, y.device)
    out = torch.empty_like(y)
    if prep["nseg"]:
        vad_launch(y, prep, out, want)
    K = prep["K"][:prep["nseg"]].cpu().numpy()
    extras = {k: prep[k][:prep["nseg" if k == "t" else "nwin"]] for k in want}
    extras["first"] = prep["first"]
    return out, K, extras


def trim_long_silences_batch(wavs: Sequence, device="cuda"):
    """trim_long_silences(wav) of every (volume-normalised, 16 kHz) utterance, one pass for all -> (list of 1-D device fp32
    tensors of 480 K[i] samples, K [n] numpy).  K[i] == 0: shorter than one window, or nothing detected."""
    arrs = [flat(w) for w in wavs]
    if not arrs:
        return [], np.zeros(0, dtype=np.int32)
    y, offs = pack(arrs, device)
    table = np.zeros((len(arrs), 6), dtype=np.int64)
    table[:, 2] = offs
    table[:, 3] = [a.shape[0] for a in arrs]
    out, K, _ = vad_packed(y, table)
    return [out[int(o):int(o) + VAD_WINDOW * int(k)] for o, k in zip(offs, K)], K


# ------------------------------------------------------------------------------------------------------------------ CLI
def _parse(argv):
    p = argparse.ArgumentParser(prog="python -m dvae_amd.preprocess",
                                description="Preprocess a VCTK wav tree into the mel corpus <out>/<speaker>/*_mel.npy "
                                            "(the reference's preprocessing/dataset_preprocess.py), on the GPU.")
    p.add_argument("datasets_root", type=Path, help="directory holding VCTK-Corpus/wav16/<speaker>/**/*.wav")
    p.add_argument("-o", "--out_dir", type=Path, default=argparse.SUPPRESS,
                   help="output directory (default <datasets_root>/SV2TTS/encoder)")
    p.add_argument("-d", "--datasets", type=str, default="VCTK", help="comma-separated dataset names (supported: VCTK)")
    p.add_argument("-s", "--skip_existing", action="store_true",
                   help="skip files already listed in <speaker>/_sources.txt (resume an interrupted run)")
    p.add_argument("--no_trim", action="store_true",
                   help="preprocess without silence trimming (one of --no_trim / --trim is required: no webrtcvad here)")
    p.add_argument("--trim", action="store_true",
                   help="trim long silences with the energy detector on the GPU (not webrtcvad: parity unpinned)")
    p.add_argument("--batch-seconds", type=float, default=1200.0,
                   help="seconds of 16 kHz output per GPU batch (a longer file goes alone); does not change any output")
    p.add_argument("--workers", type=int, default=8, help="host threads that decode and write (at most 16)")
    return p.parse_args(argv)


def main(argv=None) -> int:
    args = _parse(sys.argv[1:] if argv is None else argv)
    names = [d.strip() for d in args.datasets.split(",") if d.strip()]
    unknown = [d for d in names if d not in DATASETS]
    if unknown or not names:
        print(f"preprocess: unsupported dataset(s) {unknown or names}; supported: {', '.join(DATASETS)}", file=sys.stderr)
        return 2
    if args.trim and args.no_trim:
        print("preprocess: --trim and --no_trim exclude each other: choose one", file=sys.stderr)
        return 2
    if not args.no_trim and not args.trim:             # dataset_preprocess.py:42-50; no VAD package here
        print(f"preprocess: ModuleNotFoundError: {NO_TRIM_MESSAGE}\n"
              "preprocess: or use --trim for the energy-based trimming built into this tool.", file=sys.stderr)
        return 2
    if args.batch_seconds <= 0:
        print("preprocess: --batch-seconds must be > 0", file=sys.stderr)
        return 2
    workers = max(1, min(16, args.workers))
    out_dir = args.out_dir if hasattr(args, "out_dir") else args.datasets_root.joinpath("SV2TTS", "encoder")
    dataset_root = args.datasets_root.joinpath("VCTK-Corpus", "wav16")
    if not dataset_root.is_dir():
        print(f"preprocess: {dataset_root} does not exist", file=sys.stderr)
        return 2
    out_dir.mkdir(exist_ok=True, parents=True)
    stats = preprocess_vctk(dataset_root, out_dir, args.skip_existing, args.batch_seconds, workers, trim=args.trim)
    skipped = stats["skipped"]
    trimmed = ""
    if "trimmed_samples" in stats:
        trimmed = f"; trimmed {stats['trimmed_samples'] / SAMPLE_RATE:.1f} s of {stats['total_samples'] / SAMPLE_RATE:.1f} s"
    print(f"preprocess: {stats['written']} written, {stats['existing']} already present, {len(skipped)} skipped" + trimmed
          + "".join(f"; {p} ({why})" for p, why in skipped))
    return 0


def preprocess_vctk(dataset_root: Path, out_dir: Path, skip_existing=False, batch_seconds=1200.0, workers=8,
                    run_batch=None, decode_ahead=None, trim=False) -> dict:
    """encoder/preprocess.py:78-138 on the sorted speaker directories of `dataset_root`, in one ordered stream of
    batches over all speakers, pipelined: `workers` threads decode at most `decode_ahead` (default 4 x workers) files
    ahead of the batch being filled; each batch is resampled, normalised and turned into mels on the GPU (`run_batch`,
    default the HIP passes) while the next files decode; a separate writer pool saves it while the next batch runs, and a
    batch's `_sources.txt` lines follow once its files are on disk.  Host memory is bounded by the decode window, the
    batch being filled and the batch being written, whatever the corpus size.  `trim` selects the default runner's
    silence trimming (an injected `run_batch` does its own); where the runner counts them (`trim_stats`), the samples it
    saw and trimmed come back as total_samples / trimmed_samples."""
    speakers = sorted(d for d in dataset_root.iterdir() if d.is_dir())
    items, sources = [], {}
    existing_count = 0
    for spk in speakers:
        spk_out = out_dir.joinpath(spk.name)           # preprocess.py:86, the active line
        spk_out.mkdir(exist_ok=True)
        src = spk_out.joinpath("_sources.txt")
        existing = set()
        if skip_existing and src.exists():
            with src.open("r") as fh:
                existing = {line.split(",")[0] for line in fh}
        sources[spk.name] = src.open("a" if skip_existing else "w")
        for in_fpath in sorted(spk.glob("**/*.wav")):
            out_fname = "_".join(in_fpath.relative_to(spk).parts).replace(".wav", "_mel.npy")
            if skip_existing and out_fname in existing:
                existing_count += 1
                continue
            items.append((spk.name, in_fpath, spk_out.joinpath(out_fname), out_fname))
    written, skipped = 0, []
    limit = int(batch_seconds * SAMPLE_RATE)
    ahead = max(1, decode_ahead if decode_ahead is not None else 4 * workers)
    try:
        if items and run_batch is None:
            run_batch = _gpu_runner(trim)
        with ThreadPoolExecutor(max_workers=workers) as decoders, \
                ThreadPoolExecutor(max_workers=max(1, min(4, workers))) as writers:
            queue = deque()                            # decode futures in file order, at most `ahead` of them
            next_item = 0

            def refill():
                nonlocal next_item
                while next_item < len(items) and len(queue) < ahead:
                    queue.append(decoders.submit(read_wav, items[next_item][1], 600.0))
                    next_item += 1

            batch, size = [], 0
            pending, lines = [], []                    # the previous batch's writes and its sources lines

            def settle():
                for f in pending:                      # its files on disk, then its lines, in file order
                    f.result()
                for spk, line in lines:
                    sources[spk].write(line)
                pending.clear()
                lines.clear()

            def flush():
                nonlocal written
                if not batch:
                    return
                res = run_batch([b[1] for b in batch], [b[2] for b in batch])
                settle()
                for (it, _, _), (mel, why) in zip(batch, res):
                    if why:
                        skipped.append((str(it[1]), why))
                    else:
                        pending.append(writers.submit(_save, str(it[2]), mel))
                        lines.append((it[0], "%s,%s\n" % (it[3], it[1])))
                        written += 1
                batch.clear()

            refill()
            for it in items:
                wav, sr = queue.popleft().result()
                refill()
                if wav.shape[0] == 0:
                    skipped.append((str(it[1]), "empty"))
                    continue
                n_out = wav.shape[0] if sr == SAMPLE_RATE else resample_lengths(wav.shape[0], sr)[1]
                if sr != SAMPLE_RATE and resample_lengths(wav.shape[0], sr)[0] < 1:
                    skipped.append((str(it[1]), f"too short to resample ({wav.shape[0]} samples at {sr} Hz)"))
                    continue
                if batch and size + n_out > limit:
                    flush()
                    size = 0
                batch.append((it, wav, sr))
                size += n_out
            flush()
            settle()
    finally:
        for fh in sources.values():
            fh.close()
    stats = dict(written=written, existing=existing_count, skipped=skipped)
    counts = getattr(run_batch, "trim_stats", None)
    if counts is not None:
        stats.update(total_samples=counts["total"], trimmed_samples=counts["total"] - counts["kept"])
    return stats


def _save(path, mel):
    np.save(path, mel)


def _gpu_runner(trim=False):
    fe, rs = MelFrontend(), Resampler()
    if not trim:
        return lambda wavs, srs: _run_batch(fe, rs, wavs, srs)
    counts = dict(total=0, kept=0)                     # 16 kHz samples of the utterances written, before and after trimming

    def run(wavs, srs):
        return _run_batch(fe, rs, wavs, srs, trim=True, counts=counts)

    run.trim_stats = counts
    return run


def _run_batch(fe, rs: Resampler, wavs, srs, trim=False, counts=None):
    """one batch: resample -> normalise [-> trim] -> mel on the current stream -> list of ([80, M] float32 numpy | None,
    reason).  trim: the mel runs on the compacted buffer of vad_packed, 480 K samples per utterance; K == 0 is skipped."""
    x, _ = pack(wavs, fe.device)
    y, table = rs.packed(x, [w.shape[0] for w in wavs], srs)
    _, _, silent = volume_packed(y, table)
    out = [(None, "silent")] * len(wavs)
    lengths = table[:, 3]
    if trim:
        y, K, _ = vad_packed(y, table)
        lengths = VAD_WINDOW * K.astype(np.int64)
        for i in range(len(wavs)):
            if not silent[i] and K[i] == 0:
                out[i] = (None, TOO_SHORT_TO_TRIM if table[i, 3] < VAD_WINDOW else NO_SPEECH)
    keep = [i for i in range(len(wavs)) if not silent[i] and lengths[i] > 0]
    if counts is not None:
        counts["total"] += int(table[keep, 3].sum())
        counts["kept"] += int(lengths[keep].sum())
    if keep:
        packed, ms = fe.mel_packed(y, table[keep, 2], lengths[keep])
        for i, m in zip(keep, fe.unpack(packed.cpu().numpy(), ms)):
            out[i] = (m, None)
    return out


if __name__ == "__main__":
    sys.exit(main())
