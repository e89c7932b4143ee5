"""Over-smoothing of conversions: global variance, modulation spectrum and the modulation-spectrum postfilter (DESIGN.md
section 4.14; the kernels are csrc/modspec.hip).

A VAE decoder trained on L1 + KL averages over what its latent does not explain: the converted mel moves less from frame to
frame than natural speech does.  The classical instruments for that are the global variance (GV: the variance of each bin's
trajectory over an utterance) and the modulation spectrum (MS: the log power spectrum of each bin's trajectory over windows of
D frames); the classical repair is the MS postfilter of Takamichi et al., which moves the MS of generated trajectories onto
the statistics of natural ones.  `ModSpec.stats` measures both per group on the device, `ModSpec.score` compares two groups,
`ModSpec.postfilter` filters mels window by window and cross-fades the windows back with the conversion chain's own
overlap-add.

    python -m dvae_amd.modspec score <converted_dir> <natural_dir> [--D N] [--json PATH]

turns both directories into mels on the corpus's own path and prints `msd: <x> dB`, `gv ratio: <y> dB` (negative: the
converted files are smoother than the natural ones) and the per-modulation-frequency profile; it writes modspec.json.

No trained model and no speech corpus were available when this was written: the audible effect on real conversions is NOT
measured, and max_gain_db = 12 is a setting, not a measured optimum.
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

from ._lib import check, lib, ptr, stream
from .convert import crossfade_window, flat_plan, list_wavs, mel_to_windows, wavs_to_mels, windows_overlap_add
from .packed import upload

N_MEL = 80
SAMPLE_RATE, FRAME_HOP = 16000, 256                     # a mel frame every 256 samples at 16 kHz
D_MIN, D_MAX = 8, 128                                   # DVAE_MODSPEC_DMIN / DMAX of include/dvae_hip.h
FLOOR = 1e-30                                           # DVAE_MODSPEC_FLOOR: under |Y_k|^2, and under a variance before its ln
SIGMA_MIN = 1e-6                                        # DVAE_MODSPEC_SIGMA_MIN: a smaller sigma counts as this
DB = 10.0 / math.log(10.0)


def check_window(D, hop=None) -> tuple:
    """-> (D, hop) as ints, or ValueError: D even in [8, 128], 1 <= hop <= D (default D / 2)"""
    D = int(D)
    if D % 2 or not D_MIN <= D <= D_MAX:
        raise ValueError(f"a window of D={D} frames: D must be even and lie in [{D_MIN}, {D_MAX}]")
    hop = D // 2 if hop is None else int(hop)
    if not 1 <= hop <= D:
        raise ValueError(f"a hop of {hop} frames must lie in [1, D={D}]")
    return D, hop


def twiddle(D: int) -> np.ndarray:
    """{cos, sin}(2 pi j / D), float64 [D, 2]: the host table of the kernels (as packed.onesided_dft builds its own)"""
    ang = 2.0 * np.pi * np.arange(int(D), dtype=np.float64) / int(D)
    return np.stack([np.cos(ang), np.sin(ang)], axis=1)


def frequencies(D: int) -> np.ndarray:
    """modulation frequency of k = 1 .. D/2 in Hz"""
    return np.arange(1, int(D) // 2 + 1, dtype=np.float64) * SAMPLE_RATE / (FRAME_HOP * int(D))


def plan(lengths: Sequence[int], D: int, hop: int) -> dict:
    """convert.flat_plan with windows of D frames; an utterance with L < D has NO window here: its row of `utt` says nwin = 0
    (the overlap-add then leaves its columns alone) and its zero-padded window of the list becomes a padding window."""
    p = flat_plan(lengths, D, hop, 1)
    for u, (_, L, win0, nwin) in enumerate(p["utt"]):
        if L < D:
            p["win"][win0:win0 + nwin, 0] = -1
            p["utt"][u, 3] = 0
    p["nwin"] = int((p["win"][:, 0] >= 0).sum())
    return p


# --------------------------------------------------------------------------------------------------------- the launches
def _dev(t, dtype, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise ValueError(f"{what}: a contiguous {dtype} GPU tensor")


def mel_gv(mels, utt_table):
    """dvae_mel_gv: mels [C, ld] packed, utt_table [nutt, 4] int32 -> [nutt, C, 2] float64 (mean, population variance)"""
    _dev(mels, torch.float32, "mel_gv: mels")
    _dev(utt_table, torch.int32, "mel_gv: utt_table")
    C, ld = mels.shape
    nutt = utt_table.shape[0]
    out = torch.empty((nutt, C, 2), device=mels.device, dtype=torch.float64)
    check(lib().dvae_mel_gv(ptr(mels), ld, ptr(utt_table), nutt, C, ptr(out), stream()), "dvae_mel_gv")
    return out


def modspec_windows(windows, tw):
    """dvae_modspec_windows: windows [nwin, C, D], tw = twiddle(D) on the device -> rows [nwin C, D] fp32 (s | s^2)"""
    _dev(windows, torch.float32, "modspec_windows: windows")
    _dev(tw, torch.float64, "modspec_windows: twiddle")
    nwin, C, D = windows.shape
    rows = torch.empty((nwin * C, D), device=windows.device, dtype=torch.float32)
    check(lib().dvae_modspec_windows(ptr(windows), nwin, C, D, ptr(tw), ptr(rows), stream()), "dvae_modspec_windows")
    return rows


def modspec_group_sum(rows, order, group_first, nwin: int, C: int, D: int):
    """dvae_modspec_group_sum: rows [nwin C, D]; order [n] int32 window indices group by group, group_first [G + 1] int32
    -> sums [G, C, D] float64, each the sequential sum in the order listed"""
    _dev(rows, torch.float32, "modspec_group_sum: rows")
    _dev(order, torch.int32, "modspec_group_sum: order")
    _dev(group_first, torch.int32, "modspec_group_sum: group_first")
    G = group_first.numel() - 1
    sums = torch.empty((G, C, D), device=rows.device, dtype=torch.float64)
    check(lib().dvae_modspec_group_sum(ptr(rows), ptr(order), order.numel(), ptr(group_first), G, int(nwin), int(C), int(D),
                                       ptr(sums), stream()), "dvae_modspec_group_sum")
    return sums


def modspec_filter(windows, tw, mu_n, sigma_n, mu_g, sigma_g, alpha: float, max_gain_db: float):
    """dvae_modspec_filter: windows [nwin, C, D]; the four statistics [C, D/2] float64 on the device -> [nwin, C, D]"""
    _dev(windows, torch.float32, "modspec_filter: windows")
    nwin, C, D = windows.shape
    for t, what in ((tw, "twiddle"), (mu_n, "mu_n"), (sigma_n, "sigma_n"), (mu_g, "mu_g"), (sigma_g, "sigma_g")):
        _dev(t, torch.float64, f"modspec_filter: {what}")
        if what != "twiddle" and t.numel() != C * (D // 2):
            raise ValueError(f"modspec_filter: {what} must be [{C}, {D // 2}]")
    out = torch.empty_like(windows)
    check(lib().dvae_modspec_filter(ptr(windows), nwin, C, D, ptr(tw), ptr(mu_n), ptr(sigma_n), ptr(mu_g), ptr(sigma_g),
                                    float(alpha), float(max_gain_db), ptr(out), stream()), "dvae_modspec_filter")
    return out


# ------------------------------------------------------------------------------------------------------- the statistics
class ModSpecStats:
    """Per-group statistics of the modulation spectrum and the global variance.  Data only: for every group the float64 sums
    of s and s^2 [C, D/2] over its windows with the window count, and the float64 sums of v and ln max(v, FLOOR) [C] over its
    utterances with the utterance count.  `save` writes an .npz that `load` reads without pickle."""

    def __init__(self, names, D, hop, s_sum, s_sq, windows, v_sum, lnv_sum, utterances):
        self.names = [str(n) for n in names]
        G = len(self.names)
        self.D, self.hop = check_window(D, hop)
        f = lambda a, tail: np.ascontiguousarray(a, dtype=np.float64).reshape((G, -1) + tail)
        self.s_sum, self.s_sq = f(s_sum, (self.D // 2,)), f(s_sq, (self.D // 2,))
        self.v_sum, self.lnv_sum = f(v_sum, ()), f(lnv_sum, ())
        self.windows = np.ascontiguousarray(windows, dtype=np.int64).reshape(G)
        self.utterances = np.ascontiguousarray(utterances, dtype=np.int64).reshape(G)
        if not (self.s_sum.shape == self.s_sq.shape and self.v_sum.shape == self.lnv_sum.shape == self.s_sum.shape[:2]):
            raise ValueError("ModSpecStats: the sums disagree in their shapes")

    @property
    def C(self) -> int:
        return self.s_sum.shape[1]

    def index(self, name) -> int:
        if name not in self.names:
            raise KeyError(f"ModSpecStats: no group {name!r} (it holds {self.names})")
        return self.names.index(name)

    def _group(self, name, counts, what):
        g = self.index(name)
        if counts[g] < 1:
            raise ValueError(f"ModSpecStats: group {name!r} holds no {what} (every utterance shorter than D={self.D}?)")
        return g

    def mean(self, name) -> np.ndarray:
        """mu [C, D/2]"""
        g = self._group(name, self.windows, "window")
        return self.s_sum[g] / self.windows[g]

    def std(self, name) -> np.ndarray:
        """sigma [C, D/2], at least SIGMA_MIN"""
        g = self._group(name, self.windows, "window")
        mu = self.s_sum[g] / self.windows[g]
        return np.maximum(np.sqrt(np.maximum(self.s_sq[g] / self.windows[g] - mu * mu, 0.0)), SIGMA_MIN)

    def gv(self, name) -> np.ndarray:
        """the global variance [C]: the mean over the group's utterances of each bin's variance"""
        g = self._group(name, self.utterances, "utterance")
        return self.v_sum[g] / self.utterances[g]

    def log_gv(self, name) -> np.ndarray:
        """the mean of ln v over the group's utterances [C]"""
        g = self._group(name, self.utterances, "utterance")
        return self.lnv_sum[g] / self.utterances[g]

    def merge(self, other: "ModSpecStats") -> "ModSpecStats":
        """the statistics of the union: a group both hold has its sums added, the others are taken over"""
        if (self.D, self.hop, self.C) != (other.D, other.hop, other.C):
            raise ValueError(f"ModSpecStats.merge: D={self.D}, hop={self.hop}, C={self.C} against D={other.D}, hop={other.hop}, "
                             f"C={other.C}")
        names = self.names + [n for n in other.names if n not in self.names]
        fields = ("s_sum", "s_sq", "windows", "v_sum", "lnv_sum", "utterances")
        out = {k: np.zeros((len(names),) + getattr(self, k).shape[1:], getattr(self, k).dtype) for k in fields}
        for src in (self, other):
            for g, n in enumerate(src.names):
                for k in fields:
                    out[k][names.index(n)] += getattr(src, k)[g]
        return ModSpecStats(names, self.D, self.hop, **out)

    def save(self, path) -> str:
        path = str(path)
        path = path if path.endswith(".npz") else path + ".npz"
        np.savez(path, names=np.asarray(self.names, dtype=np.str_), D=np.int64(self.D), hop=np.int64(self.hop),
                 s_sum=self.s_sum, s_sq=self.s_sq, windows=self.windows, v_sum=self.v_sum, lnv_sum=self.lnv_sum,
                 utterances=self.utterances)
        return path

    @classmethod
    def load(cls, path) -> "ModSpecStats":
        with np.load(str(path), allow_pickle=False) as f:
            return cls([str(n) for n in f["names"]], int(f["D"]), int(f["hop"]), f["s_sum"], f["s_sq"], f["windows"],
                       f["v_sum"], f["lnv_sum"], f["utterances"])


def score_stats(stats_a: ModSpecStats, name_a, stats_b: ModSpecStats, name_b) -> dict:
    """msd_db = (10 / ln 10) sqrt(mean over c, k of (mu_a - mu_b)^2); gv_ratio_db = (10 / ln 10) mean_c(mean ln v_a - mean ln v_b),
    negative when a is smoother than b; profile[k] = mean_c(mu_a - mu_b) at frequencies_hz[k] (a difference of ln power;
    profile_db the same in dB).  Host arithmetic on the sums."""
    if (stats_a.D, stats_a.C) != (stats_b.D, stats_b.C):
        raise ValueError(f"score: statistics of D={stats_a.D}, C={stats_a.C} against D={stats_b.D}, C={stats_b.C}")
    diff = stats_a.mean(name_a) - stats_b.mean(name_b)
    return dict(msd_db=float(DB * np.sqrt(np.mean(diff * diff))),
                gv_ratio_db=float(DB * np.mean(stats_a.log_gv(name_a) - stats_b.log_gv(name_b))),
                profile=diff.mean(axis=0), profile_db=DB * diff.mean(axis=0), frequencies_hz=frequencies(stats_a.D))


# ----------------------------------------------------------------------------------------------------------- the engine
class ModSpec:
    """The instruments on one device, for windows of D frames `hop` apart (default D / 2): independent of the model's T."""

    def __init__(self, device, D: int = 64, hop=None):
        self.D, self.hop = check_window(D, hop)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ModSpec runs on the HIP path only (no CPU fallback)")
        self.tw = upload(twiddle(self.D), self.device, np.float64)
        self.window = upload(crossfade_window(self.D), self.device)

    def _mels(self, mels):
        ms = [torch.as_tensor(m).to(self.device, torch.float32) for m in mels]
        if not ms:
            raise ValueError("modspec: no mel")
        C = ms[0].shape[0] if ms[0].dim() == 2 else 0
        for m in ms:
            if m.dim() != 2 or m.shape[0] != C or m.shape[1] < 1 or C < 1:
                raise ValueError(f"modspec: every mel must be [{C or 'C'}, L >= 1], not {tuple(m.shape)}")
        return ms

    def pack(self, mels: Sequence):
        """list of [C, L] -> (plan with the tables on the device as plan['utt_d'], plan['win_d'], packed [C, ld])"""
        ms = self._mels(mels)
        p = plan([int(m.shape[1]) for m in ms], self.D, self.hop)
        packed = torch.zeros((ms[0].shape[0], p["ld"]), device=self.device, dtype=torch.float32)
        for m, (col0, L, _, _) in zip(ms, p["utt"]):
            packed[:, col0:col0 + L] = m
        p["utt_d"] = upload(p["utt"], self.device, np.int32)
        p["win_d"] = upload(p["win"], self.device, np.int32)
        return p, packed

    def stats(self, mels_by_name: dict) -> ModSpecStats:
        """{name: [mel [C, L], ...]} -> ModSpecStats.  An utterance with L < D enters no statistic."""
        names = list(mels_by_name)
        mels, owner = [], []
        for g, name in enumerate(names):
            group = mels_by_name[name]
            group = [group] if (torch.is_tensor(group) or isinstance(group, np.ndarray)) and group.ndim == 2 else list(group)
            mels += group
            owner += [g] * len(group)
        if not mels:
            raise ValueError("modspec.stats: no utterance")
        G, H = len(names), self.D // 2
        owner = np.asarray(owner, dtype=np.int64)
        p, packed = self.pack(mels)
        C = packed.shape[0]
        s_sums, windows = np.zeros((G, C, self.D)), np.zeros(G, dtype=np.int64)
        wg = np.where(p["win"][:, 0] >= 0, owner[np.maximum(p["win"][:, 0], 0)], -1)
        order = np.concatenate([np.nonzero(wg == g)[0] for g in range(G)])
        if order.size:
            windows = np.asarray([(wg == g).sum() for g in range(G)], dtype=np.int64)
            first = np.concatenate([[0], np.cumsum(windows)])
            rows = modspec_windows(mel_to_windows(packed, p["utt_d"], p["win_d"], self.D), self.tw)
            s_sums = modspec_group_sum(rows, upload(order, self.device, np.int32), upload(first, self.device, np.int32),
                                       len(p["win"]), C, self.D).cpu().numpy()
        gv = mel_gv(packed, p["utt_d"]).cpu().numpy()
        v_sum, lnv_sum, utts = np.zeros((G, C)), np.zeros((G, C)), np.zeros(G, dtype=np.int64)
        for u, g in enumerate(owner):                       # float64, in utterance order
            if p["utt"][u, 1] >= self.D:
                v_sum[g] += gv[u, :, 1]
                lnv_sum[g] += np.log(np.maximum(gv[u, :, 1], FLOOR))
                utts[g] += 1
        return ModSpecStats(names, self.D, self.hop, s_sums[:, :, :H], s_sums[:, :, H:], windows, v_sum, lnv_sum, utts)

    def score(self, stats_a: ModSpecStats, name_a, stats_b: ModSpecStats, name_b) -> dict:
        return score_stats(stats_a, name_a, stats_b, name_b)

    def _check_stats(self, pair, what):
        st, name = pair
        if st.D != self.D:
            raise ValueError(f"postfilter: the {what} statistics are of windows of D={st.D}, this ModSpec cuts D={self.D}")
        return st.mean(name), st.std(name)

    def postfilter(self, mels: Sequence, natural, generated, alpha: float = 1.0, max_gain_db: float = 12.0) -> list:
        """mels: list of [C, L]; natural, generated: (ModSpecStats, name).  -> list of [C, L] on the device, the input's frame
        counts: every window of D frames filtered (dvae_modspec_filter), the windows cross-faded back with crossfade_window(D)
        and clamped to [0, 1] by dvae_windows_overlap_add.  alpha = 0 returns the input's bits; so does an utterance with
        L < D at any alpha."""
        alpha, max_gain_db = float(alpha), float(max_gain_db)
        if not 0.0 <= alpha <= 1.0 or not max_gain_db > 0.0:
            raise ValueError(f"postfilter: alpha={alpha} must lie in [0, 1] and max_gain_db={max_gain_db} be positive")
        (mu_n, sg_n), (mu_g, sg_g) = self._check_stats(natural, "natural"), self._check_stats(generated, "generated")
        ms = self._mels(mels)
        if mu_n.shape != (ms[0].shape[0], self.D // 2) or mu_g.shape != mu_n.shape:
            raise ValueError(f"postfilter: statistics of {mu_n.shape[0]} and {mu_g.shape[0]} bins, mels of {ms[0].shape[0]}")
        p, packed = self.pack(ms)
        if alpha == 0.0 or p["nwin"] == 0:
            return [m.clone() for m in ms]
        up = lambda a: upload(a, self.device, np.float64)
        y = modspec_filter(mel_to_windows(packed, p["utt_d"], p["win_d"], self.D), self.tw, up(mu_n), up(sg_n), up(mu_g),
                           up(sg_g), alpha, max_gain_db)
        out = windows_overlap_add(y, p["utt_d"], p["win_d"], self.window, p["ld"], clamp=(0.0, 1.0), out=packed.clone())
        return [out[:, col0:col0 + L].contiguous() for col0, L, _, _ in p["utt"]]


# ---------------------------------------------------------------------------------------------------------- the command
def _parse(argv):
    p = argparse.ArgumentParser(prog="python -m dvae_amd.modspec",
                                description="Over-smoothing scores of converted .wav files against natural ones: modulation-"
                                            "spectrum distance and global-variance ratio, on the GPU.")
    sub = p.add_subparsers(dest="command", required=True)
    s = sub.add_parser("score", help="msd and gv ratio of <converted_dir> against <natural_dir>")
    s.add_argument("converted_dir", type=Path, help="directory of converted *.wav")
    s.add_argument("natural_dir", type=Path, help="directory of natural *.wav of the target speaker")
    s.add_argument("--D", type=int, default=64, help="frames per analysis window (even, 8 ... 128)")
    s.add_argument("--json", type=Path, default=None, help="where to write the results (default <converted_dir>/modspec.json)")
    return p.parse_args(argv)


def main(argv=None) -> int:
    args = _parse(sys.argv[1:] if argv is None else argv)
    report = lambda msg: print(f"modspec: {msg}", file=sys.stderr)
    try:
        check_window(args.D)
    except ValueError as e:
        report(str(e))
        return 2
    for d in (args.converted_dir, args.natural_dir):
        if not d.is_dir():
            report(f"{d} is not a directory")
            return 2
    if not torch.cuda.is_available():
        report("no GPU: the modulation spectrum runs on the HIP path only")
        return 2
    from .frontend import MelFrontend
    from .preprocess import Resampler
    device = torch.device("cuda", torch.cuda.current_device())
    fe, rs, ms = MelFrontend(device), Resampler(device), ModSpec(device, args.D)
    result = dict(converted_dir=str(args.converted_dir), natural_dir=str(args.natural_dir), D=ms.D, hop=ms.hop, msd_db=None,
                  gv_ratio_db=None, frequencies_hz=frequencies(ms.D).tolist(), profile=None, windows={}, utterances={},
                  unusable={}, too_short={})
    groups = {}
    for side, d in (("converted", args.converted_dir), ("natural", args.natural_dir)):
        skipped = []
        got = wavs_to_mels(list_wavs([d]), fe, rs, lambda msg: (skipped.append(msg), report(msg)))
        result["unusable"][side] = skipped
        result["too_short"][side] = [str(q) for q, mel, _ in got if mel.shape[1] < ms.D]
        for q in result["too_short"][side]:
            report(f"skipped {q}: fewer than {ms.D} frames")
        groups[side] = [mel for _, mel, _ in got if mel.shape[1] >= ms.D]
    out_path = args.json or args.converted_dir.joinpath("modspec.json")
    empty = [side for side, g in groups.items() if not g]
    if empty:
        report(f"no usable file of at least {ms.D} frames in the {' and the '.join(empty)} directory")
        out_path.write_text(json.dumps(result, indent=1) + "\n")
        return 1
    st = ms.stats(groups)
    sc = ms.score(st, "converted", st, "natural")
    result.update(msd_db=sc["msd_db"], gv_ratio_db=sc["gv_ratio_db"], profile=sc["profile"].tolist(),
                  profile_db=sc["profile_db"].tolist(),
                  windows={n: int(st.windows[st.index(n)]) for n in st.names},
                  utterances={n: int(st.utterances[st.index(n)]) for n in st.names})
    print(f"msd: {sc['msd_db']} dB")
    print(f"gv ratio: {sc['gv_ratio_db']} dB")
    for f, v in zip(sc["frequencies_hz"], sc["profile_db"]):
        print(f"profile {f:.3f} Hz: {v} dB")
    out_path.write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
