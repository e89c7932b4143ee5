"""The packed-batch layer under the audio tools (mel front-end, Griffin-Lim inverse, corpus preprocessing, MCD scoring).

One format: a ragged batch of utterances lies back to back in one device buffer, every utterance at a 16-byte aligned
start (`pack`); its frames are the rows of one `[sum M, ...]` matrix (`pack_rows`, `split_rows`); a small int64 table
`{row0, M, sample0, n}` per utterance (`segment_table`) tells the segmented HIP passes of csrc/frontend.hip which rows
and samples belong together.  One policy: a contraction between those passes runs with fp32 products and ONE k-split
(`pinned_gemm`), so a row's bits do not depend on what shares its batch.  And the host tables those contractions read
(one-sided DFT cos/sin, the periodic Hann window), float64 until `upload`.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import ops


def pad4(n: int) -> int:
    """n rounded up to 4 elements (16 bytes of fp32)"""
    return (n + 3) // 4 * 4


def padded_bins(fft_size: int) -> int:
    """the one-sided bin count fft_size / 2 + 1, padded so that rows of bins stay 16-byte aligned"""
    return pad4(fft_size // 2 + 1)


# ------------------------------------------------------------------------------------------------ host tables (float64)
def hann_periodic(n: int) -> np.ndarray:
    k = np.arange(n, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * k / n)


def onesided_dft(fft_size: int, rows=None, inverse: bool = False):
    """(cos, sin) of 2 pi k j / N, float64 [len(rows), nb]: k over `rows` (default 0..N-1), j over the nb = N/2 + 1
    one-sided bins.  inverse: both scaled by c_j / N with c_0 = c_{N/2} = 1, c_j = 2 otherwise, the weights with which
    a real signal comes back from its one-sided spectrum (np.fft.irfft).  The angle matrix is symmetric in (k, j), so
    the forward basis over all k is the transpose."""
    nb = fft_size // 2 + 1
    k = np.arange(fft_size, dtype=np.float64) if rows is None else np.asarray(rows, dtype=np.float64)
    ang = 2.0 * np.pi * np.outer(k, np.arange(nb, dtype=np.float64)) / fft_size
    if not inverse:
        return np.cos(ang), np.sin(ang)
    c = np.full(nb, 2.0)
    c[0] = 1.0
    if fft_size % 2 == 0:
        c[-1] = 1.0
    return c / fft_size * np.cos(ang), c / fft_size * np.sin(ang)


def upload(a, device, dtype=np.float32):
    """host table -> contiguous device tensor of `dtype` (float32, int32 or int64)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)


# ------------------------------------------------------------------------------------------------------ packing samples
def flat(wav):
    """one waveform (array-like or tensor) -> 1-D: a float32 numpy array, or the tensor flattened where it is"""
    return wav.reshape(-1) if torch.is_tensor(wav) else np.asarray(wav, dtype=np.float32).reshape(-1)


def pack(arrays: Sequence, device="cuda"):
    """list of 1-D float32 arrays / tensors -> (device fp32 buffer, offsets): each starts at a multiple of 4 elements (the
    packing of dvae_resample_segment_table)"""
    ns = [int(a.shape[0]) for a in arrays]
    offs = np.zeros(len(ns), dtype=np.int64)
    tot = 0
    for i, n in enumerate(ns):
        offs[i] = tot
        tot += pad4(n)
    if all(not torch.is_tensor(a) for a in arrays):
        host = np.zeros(max(4, tot), dtype=np.float32)
        for a, o, n in zip(arrays, offs, ns):
            host[o:o + n] = a
        return torch.from_numpy(host).to(device), offs
    buf = torch.zeros(max(4, tot), device=device, dtype=torch.float32)
    for a, o, n in zip(arrays, offs, ns):
        buf[o:o + n] = torch.as_tensor(a).to(device, torch.float32).view(-1)
    return buf, offs


def segment_table(frames: Sequence[int], sample0: Sequence[int], lengths: Sequence[int]) -> np.ndarray:
    """[nseg, 4] int64 {row0, M, sample0, n}: utterance s owns rows [row0, row0 + M) of the packed frame matrix and
    samples [sample0, sample0 + n) of the packed buffer (the layout dvae_gl_segment_table writes)"""
    table = np.zeros((len(frames), 4), dtype=np.int64)
    table[:, 1] = frames
    table[1:, 0] = np.cumsum(table[:-1, 1])
    table[:, 2] = sample0
    table[:, 3] = lengths
    return table


# --------------------------------------------------------------------------------------------------------- packing rows
def pack_rows(seqs: Sequence, width: int, device="cuda"):
    """list of [n_i, <= width] arrays / tensors -> ([max(1, sum n_i), width] device fp32 with the sequences back to back,
    zero right of a narrower one; row0 [nseq] int64; [n_i]).  All numpy: assembled on the host, one copy."""
    ns = [int(s.shape[0]) for s in seqs]
    row0 = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
    if all(not torch.is_tensor(s) for s in seqs):
        out = np.zeros((max(1, sum(ns)), width), dtype=np.float32)
    else:
        out = torch.zeros((max(1, sum(ns)), width), device=device, dtype=torch.float32)
    for s, r, n in zip(seqs, row0, ns):
        out[r:r + n, :s.shape[1]] = s
    return (out if torch.is_tensor(out) else torch.from_numpy(out).to(device)), row0, ns


def split_rows(x, counts: Sequence[int]) -> list:
    """packed [sum counts, ...] (tensor or array) -> list of views [counts[i], ...]"""
    ends = np.cumsum(counts)
    return [x[int(e - m):int(e)] for e, m in zip(ends, counts)]


# ---------------------------------------------------------------------------------------------------------- contraction
def pinned_gemm(A, B, C, K, act=ops.ACT_NONE):
    """C[rows, N] = act(A[rows, K] B[N, K]^T) with fp32 products and ONE k-split whatever the row count: the bits of a row
    do not depend on the batch it shares a launch with, on the training compute mode or on ops.set_deterministic"""
    ops.gemm(A, B, C, None, A.shape[0], B.shape[0], K, K, K, B.shape[0], True, True, act, ops.EPI_STORE, 1, ops.MODE_F32)
