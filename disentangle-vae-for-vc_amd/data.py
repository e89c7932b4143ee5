"""Feeder of the training step: same-speaker utterance pairs of mel segments.

`SpeechDatasetGVAE` keeps the semantics of /root/reference/preprocessing/dataset.py:53-123:
directory layout `<root>/<speaker>/*.npy` with arrays [80, L]; per speaker the utterance list is
shuffled, cut into two halves and the i-th files of each half form a pair (:63-76, re-done by
`shuffle_data()` each epoch :78-91); each item is cropped to `samples_length` frames at a random
offset, or right-padded with zeros when shorter (:100-109); the label is the index of the speaker
directory (:111-112).  Differences: an explicit RNG (reproducible), sorted directory listing, and
L == samples_length crops at 0 instead of raising (np.random.choice(0) in the reference).

`SyntheticPairs` is the generator used by bench.py / tests: U[0,1) mels (the range produced by
preprocessing/encoder/utils.py:132-133) already resident on the device.
"""
from __future__ import annotations

import glob
import json
import os
import zlib
from typing import Optional

import numpy as np
import torch
from torch.utils.data import Dataset


class SpeechDatasetGVAE(Dataset):
    def __init__(self, file_path, sr=16000, samples_length=64, seed: Optional[int] = None, exclude=None):
        """exclude: files (paths as `split_corpus` returns them, or a dict speaker -> such paths) that never enter `spk_utt`:
        the held-out part of the corpus.  `speaker_ids`, and with them the labels, stay those of the whole directory listing."""
        self.file_path = file_path
        self.sr = sr
        self.samples_length = samples_length
        self.rng = np.random.RandomState(seed) if seed is not None else np.random
        self.speaker_ids = self.list_speakers(file_path)
        self.spk_utt = [np.array(sorted(glob.glob(os.path.join(file_path, s, "*.npy")))) for s in self.speaker_ids]
        if exclude is not None:
            out = {os.path.abspath(f) for f in _flat_files(exclude)}
            self.spk_utt = [np.array([f for f in utt if os.path.abspath(f) not in out], dtype=utt.dtype)
                            for utt in self.spk_utt]
        self.utterance_fp = np.empty((0, 2), dtype=object)
        self.shuffle_data()

    @staticmethod
    def list_speakers(file_path):
        return sorted(d for d in os.listdir(file_path) if os.path.isdir(os.path.join(file_path, d)))

    def shuffle_data(self):
        pairs = []
        for utt in self.spk_utt:
            self.rng.shuffle(utt)
            half = utt.shape[0] // 2
            pairs += [(utt[i], utt[half + i]) for i in range(half)]
        self.utterance_fp = np.array(pairs, dtype=object).reshape(-1, 2)

    def _crop(self, mel):
        T = self.samples_length
        L = mel.shape[1]
        if L < T:
            return np.pad(mel, ((0, 0), (0, T - L)), "constant", constant_values=0)
        start = int(self.rng.randint(0, L - T)) if L > T else 0
        return mel[:, start:start + T]

    def __getitem__(self, index):
        u1, u2 = self.utterance_fp[index]
        mel1, mel2 = self._crop(np.load(u1)), self._crop(np.load(u2))
        spk = self.speaker_ids.index(os.path.basename(os.path.dirname(u1)))
        return torch.from_numpy(np.ascontiguousarray(mel1)), torch.from_numpy(np.ascontiguousarray(mel2)), \
            torch.tensor(spk)

    def __len__(self):
        return len(self.utterance_fp)

    def get_utterance(self, speaker, utterance):
        return np.load(os.path.join(self.file_path, speaker, utterance))


def _flat_files(held):
    if isinstance(held, dict):
        return [f for fs in held.values() for f in fs]
    return list(held)


# ------------------------------------------------------------------ the held-out split
def split_corpus(root, val_fraction=0.0, val_speakers=(), seed=0):
    """The held-out files of `<root>/<speaker>/*.npy`: dict speaker -> sorted list of paths (speakers with nothing held out
    are left out).  The rule depends on the sorted speaker directories, the sorted file names and `seed` alone (not on the
    training seed, not on the order a directory is listed in): per speaker the sorted files are permuted with
    RandomState(seed ^ crc32(speaker)) and the first k are held out, k = floor(val_fraction n) rounded down to an even
    number (validation pairs file i with file k/2 + i).  A speaker named in `val_speakers` is held out whole; an odd last
    file of it is dropped from validation AND excluded from training (`excluded_files`)."""
    return _split(root, val_fraction, val_speakers, seed)[0]


def _split(root, val_fraction, val_speakers, seed):
    val_fraction = float(val_fraction)
    if not 0.0 <= val_fraction < 0.5:
        raise ValueError(f"val_fraction {val_fraction}: expected 0 <= val_fraction < 0.5")
    speakers = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))
    val_speakers = tuple(val_speakers or ())
    unknown = sorted(set(val_speakers) - set(speakers))
    if unknown:
        raise ValueError(f"val_speakers {unknown}: no such speaker directory under {root}")
    held, dropped = {}, []
    for spk in speakers:
        files = sorted(glob.glob(os.path.join(root, spk, "*.npy")))
        n = len(files)
        if spk in val_speakers:
            take = files[:n - (n & 1)]
            dropped += files[n - (n & 1):]
        else:
            k = int(np.floor(val_fraction * n)) & ~1
            rs = np.random.RandomState((int(seed) ^ zlib.crc32(spk.encode("utf-8"))) & 0xFFFFFFFF)
            take = sorted(files[i] for i in rs.permutation(n)[:k])
        if take:
            held[spk] = take
    return held, dropped


def excluded_files(root, val_fraction=0.0, val_speakers=(), seed=0):
    """What training must not see: the held-out files of `split_corpus` plus the odd last file of each `val_speakers`
    speaker (dropped from validation, not trained on either)."""
    held, dropped = _split(root, val_fraction, val_speakers, seed)
    return _flat_files(held) + dropped


def write_val_split(path, root, held, excluded, val_fraction, val_speakers, val_seed):
    """`<log_dir>/val_split.json`: the held-out files relative to the corpus root, and the three settings that made them."""
    rel = lambda f: os.path.relpath(f, root).replace(os.sep, "/")
    rec = {"val_fraction": float(val_fraction), "val_speakers": sorted(val_speakers), "val_seed": int(val_seed),
           "held_out": {spk: [rel(f) for f in fs] for spk, fs in held.items()},
           "excluded": sorted(rel(f) for f in excluded)}
    with open(path, "w") as fp:
        json.dump(rec, fp, indent=1)
    return rec


def read_val_split(path, root, val_fraction, val_speakers, val_seed):
    """-> (held, excluded) with absolute paths, from the file a first run wrote.  A resumed run whose flags disagree with it
    would train on files the earlier epochs validated on: SystemExit, saying which setting differs."""
    with open(path) as fp:
        rec = json.load(fp)
    want = {"val_fraction": float(val_fraction), "val_speakers": sorted(val_speakers), "val_seed": int(val_seed)}
    diff = [f"{k}: {rec.get(k)!r} there, {v!r} now" for k, v in want.items() if rec.get(k) != v]
    if diff:
        raise SystemExit(f"{path} was written with another held-out split ({'; '.join(diff)}): a changed split would leak "
                         "validation data into training.  Use the same --val-fraction / --val-speakers / --val-seed, or "
                         "another --log_dir.")
    full = lambda r: os.path.join(root, *r.split("/"))
    return {spk: [full(r) for r in fs] for spk, fs in rec["held_out"].items()}, [full(r) for r in rec["excluded"]]


class HeldOutPairs:
    """The fixed pair list of a held-out split, resident on the device.  Per speaker the held-out files in sorted order,
    file i paired with file k/2 + i; never shuffled.  The crop is centred (start (L - T) // 2 when L > T; otherwise start 0
    and zeros on the right, the dataset's rule), made by the gather kernel of GpuPairLoader from mels uploaded once.
    `batches(batch_size)` yields (x1, x2, speaker index int32 on the device); the last batch may be short, no pair is
    dropped.  device=None builds the lists only (pairs, offsets, speakers) and uploads nothing."""

    def __init__(self, held, samples_length, speaker_ids, device="cuda"):
        self.T = int(samples_length)
        self.speaker_ids = list(speaker_ids)
        self.pairs, spk = [], []
        for name in sorted(held):
            files = sorted(held[name])
            half = len(files) // 2
            self.pairs += [(files[i], files[half + i]) for i in range(half)]
            spk += [self.speaker_ids.index(name)] * half
        self.speakers = np.array(spk, dtype=np.int32)
        files = sorted({f for p in self.pairs for f in p})
        self.index = {f: i for i, f in enumerate(files)}
        arrs = [np.load(f) for f in files]
        self.lengths = np.array([a.shape[1] for a in arrs], dtype=np.int32)
        self.offsets = np.array([(int(L) - self.T) // 2 if L > self.T else 0 for L in self.lengths], dtype=np.int32)
        self.u1 = np.array([self.index[a] for a, _ in self.pairs], dtype=np.int32)
        self.u2 = np.array([self.index[b] for _, b in self.pairs], dtype=np.int32)
        self.device = None if device is None else torch.device(device)
        if self.device is None or not arrs:
            return
        self.C, self.Lmax = arrs[0].shape[0], int(self.lengths.max())
        host = np.zeros((len(arrs), self.C, self.Lmax), dtype=np.float32)
        for i, a in enumerate(arrs):
            host[i, :, :a.shape[1]] = a
        self.mels = torch.from_numpy(host).to(self.device)
        self.lens_dev = torch.from_numpy(self.lengths).to(self.device)
        self.spk_dev = torch.from_numpy(self.speakers).to(self.device)

    def __len__(self):
        return len(self.pairs)

    def _gather(self, utt):
        from ._lib import check, lib, ptr, stream
        u = torch.from_numpy(np.ascontiguousarray(utt)).to(self.device)
        o = torch.from_numpy(np.ascontiguousarray(self.offsets[utt])).to(self.device)
        out = torch.empty((len(utt), self.C, self.T), device=self.device, dtype=torch.float32)
        check(lib().dvae_gather_crop(ptr(self.mels), ptr(self.lens_dev), ptr(u), ptr(o), ptr(out), len(utt), self.C, self.T,
                                     self.Lmax, stream()), "dvae_gather_crop")
        return out

    def batches(self, batch_size):
        if self.device is None:
            raise RuntimeError("HeldOutPairs(device=None) holds the pair list only")
        for lo in range(0, len(self.pairs), int(batch_size)):
            hi = min(lo + int(batch_size), len(self.pairs))
            yield self._gather(self.u1[lo:hi]), self._gather(self.u2[lo:hi]), self.spk_dev[lo:hi]


def write_synthetic_corpus(root, n_speakers=2, n_utt=8, n_mel=80, length=96, seed=0):
    """BASELINE config[0]: `n_speakers` x `n_utt` float64 .npy files of shape [80, length], U[0,1)."""
    rs = np.random.RandomState(seed)
    for s in range(n_speakers):
        d = os.path.join(root, f"spk{s:03d}")
        os.makedirs(d, exist_ok=True)
        for u in range(n_utt):
            np.save(os.path.join(d, f"utt{u:03d}_mel.npy"), rs.uniform(0.0, 1.0, size=(n_mel, length)))
    return root


class SyntheticPairs:
    """Device-resident synthetic batches: x1, x2 ~ U[0,1) fp32 [B, 80, T]; speaker ids uniform over n_speakers
    (ids are unused by the loss, variational_base_vae.py:58)."""

    def __init__(self, batch, n_frames, n_speakers=10, seed=1234, device="cuda", n_mel=80):
        rs = np.random.RandomState(seed)
        self.x1 = torch.from_numpy(rs.uniform(0, 1, size=(batch, n_mel, n_frames)).astype(np.float32)).to(device)
        self.x2 = torch.from_numpy(rs.uniform(0, 1, size=(batch, n_mel, n_frames)).astype(np.float32)).to(device)
        self.spk = torch.from_numpy(rs.randint(0, n_speakers, size=(batch,))).to(device)

    def batch(self):
        return self.x1, self.x2, self.spk


class GpuPairLoader:
    """Device-resident replacement for `DataLoader(SpeechDatasetGVAE, shuffle=True)` (train.py:55-56).

    With a ~36 ms step the reference's loader (num_workers=0, two np.load + a host->device copy per item) would
    dominate, so the whole corpus is uploaded ONCE as a padded [n_utt, 80, Lmax] fp32 tensor (VCTK mels are a few
    GB: trivial against 288 GB of HBM) and a batch is produced by one HIP gather kernel.  Pairing, per-epoch
    re-pairing (`dataset.shuffle_data()`), random crop / right zero-pad and the speaker label are those of
    SpeechDatasetGVAE — the pair list IS the dataset's; only where the bytes live and who crops changes.
    Yields (x1 [B,80,T], x2 [B,80,T], speaker_ids [B]) on the device.

    Data parallel: with `world_size` > 1 every rank holds the whole corpus (it is small) and takes pairs
    rank, rank+world, ... of the SAME epoch permutation, so `seed` (and the dataset's seed) must be given and equal
    on all ranks; every rank sees the same number of batches (the remainder is dropped)."""

    def __init__(self, dataset: SpeechDatasetGVAE, batch_size: int, device="cuda", seed: Optional[int] = None,
                 drop_last: bool = True, shuffle: bool = True, rank: int = 0, world_size: int = 1):
        if world_size > 1 and seed is None:
            raise ValueError("GpuPairLoader: data-parallel sharding needs an explicit seed shared by all ranks")
        if not 0 <= rank < world_size:
            raise ValueError("GpuPairLoader: rank out of range")
        self.dataset = dataset
        self.batch_size, self.drop_last, self.shuffle = batch_size, drop_last, shuffle
        self.rank, self.world_size = rank, world_size
        self.rng = np.random.RandomState(seed) if seed is not None else np.random
        self.crop_rng = np.random.RandomState(seed + 7919 * (rank + 1)) if seed is not None else np.random
        self.T = dataset.samples_length
        files = sorted({f for utts in dataset.spk_utt for f in utts})
        self.index = {f: i for i, f in enumerate(files)}
        arrs = [np.load(f) for f in files]
        self.C = arrs[0].shape[0]
        self.lengths = np.array([a.shape[1] for a in arrs], dtype=np.int32)
        self.Lmax = int(self.lengths.max())
        host = np.zeros((len(arrs), self.C, self.Lmax), dtype=np.float32)
        for i, a in enumerate(arrs):
            host[i, :, :a.shape[1]] = a
        self.device = torch.device(device)
        self.mels = torch.from_numpy(host).to(self.device)
        self.lens_dev = torch.from_numpy(self.lengths).to(self.device)
        self.last_meta = None       # (utt1, utt2, off1, off2) of the last batch, for tests

    def _n_local(self):
        return len(self.dataset) // self.world_size

    def __len__(self):
        n = self._n_local()
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _offset(self, L):
        # same rule as SpeechDatasetGVAE._crop: random start if longer, 0 (and zero padding) otherwise
        return int(self.crop_rng.randint(0, L - self.T)) if L > self.T else 0

    def gather(self, utt, off):
        """Crop batch on the device: utt, off int arrays [n] -> [n, 80, T]."""
        from ._lib import check, lib, ptr, stream
        n = len(utt)
        u = torch.as_tensor(np.asarray(utt, dtype=np.int32)).to(self.device)
        o = torch.as_tensor(np.asarray(off, dtype=np.int32)).to(self.device)
        out = torch.empty((n, self.C, self.T), device=self.device, dtype=torch.float32)
        check(lib().dvae_gather_crop(ptr(self.mels), ptr(self.lens_dev), ptr(u), ptr(o), ptr(out), n, self.C, self.T,
                                     self.Lmax, stream()), "dvae_gather_crop")
        return out

    def sample_batch(self, seed: int = 0):
        """One batch drawn with a PRIVATE generator: leaves the epoch permutation and crop streams untouched, so a rank
        that looks at a batch on its own (rank 0's estimate_trained_model) stays in step with its peers."""
        rs = np.random.RandomState(seed)
        n = len(self.dataset)
        sel = rs.permutation(n)[:min(self.batch_size, n)]
        pairs = self.dataset.utterance_fp[sel]
        u1 = np.array([self.index[p[0]] for p in pairs], dtype=np.int32)
        u2 = np.array([self.index[p[1]] for p in pairs], dtype=np.int32)
        off = lambda us: np.array([int(rs.randint(0, int(self.lengths[u]) - self.T)) if self.lengths[u] > self.T else 0
                                   for u in us], dtype=np.int32)
        spk = np.array([self.dataset.speaker_ids.index(os.path.basename(os.path.dirname(p[0]))) for p in pairs])
        return self.gather(u1, off(u1)), self.gather(u2, off(u2)), torch.from_numpy(spk).to(self.device)

    def _epoch_plan(self):
        """One epoch's batches as host arrays (utt1, utt2, off1, off2, speaker), drawn from the seeded streams in THE order an
        epoch draws them: the permutation first, then per batch the crop offsets of the x1 half and of the x2 half.  `__iter__`
        gathers them on the device; `skip_epochs` only draws."""
        n = len(self.dataset)
        order = self.rng.permutation(n) if self.shuffle else np.arange(n)     # identical on every rank
        order = order[:self._n_local() * self.world_size][self.rank::self.world_size]
        for b in range(len(self)):
            sel = order[b * self.batch_size:(b + 1) * self.batch_size]
            pairs = self.dataset.utterance_fp[sel]
            u1 = np.array([self.index[p[0]] for p in pairs], dtype=np.int32)
            u2 = np.array([self.index[p[1]] for p in pairs], dtype=np.int32)
            o1 = np.array([self._offset(int(self.lengths[u])) for u in u1], dtype=np.int32)
            o2 = np.array([self._offset(int(self.lengths[u])) for u in u2], dtype=np.int32)
            spk = np.array([self.dataset.speaker_ids.index(os.path.basename(os.path.dirname(p[0]))) for p in pairs])
            yield u1, u2, o1, o2, spk

    def skip_epochs(self, epochs: int):
        """Advance the seeded streams (the epoch permutation, the crop offsets, the dataset's re-pairing) past `epochs` whole
        epochs without touching the device: what a resumed run calls so that epoch e feeds the batches the uninterrupted run
        fed in epoch e.  Without a seed the streams are numpy's global ones and there is nothing to replay."""
        if self.rng is np.random:
            return
        for _ in range(int(epochs)):
            for _ in self._epoch_plan():
                pass
            self.dataset.shuffle_data()      # what train() does at the end of an epoch

    def __iter__(self):
        for u1, u2, o1, o2, spk in self._epoch_plan():
            self.last_meta = (u1, u2, o1, o2)
            yield self.gather(u1, o1), self.gather(u2, o2), torch.from_numpy(spk).to(self.device)
