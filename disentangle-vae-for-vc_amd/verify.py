"""GMM-UBM speaker verification of conversions on the GPU: does a converted file sound like the target
SPEAKER?  (`evaluate` says how close it is to the target utterance; `probe --score` is the model's own encoder's view.)

    python -m dvae_amd.verify train <wav16_root> -o ubm.npz [--components 64] [--iters 10] [--max-utts-per-speaker 40]
           [--seed 0]
    python -m dvae_amd.verify score <converted_dir> --ubm ubm.npz --target <wav dir> --source <wav dir>
           [--enroll-utts 20] [--relevance 16] [--json PATH]

The classical instrument (Reynolds, Quatieri, Dunn 2000), no pretrained weights and no second network:

    features   the voiced frames' mel-cepstral coefficients 1..23 of evaluate.MelCepstrum.packed, read in place (c0 is
               loudness and is dropped; no mean normalisation, no deltas: the voiced frames are compacted)
    UBM        a diagonal-covariance Gaussian mixture fitted by EM on ONE packed buffer of the corpus's frames: one
               dvae_gmm_estep call per iteration (fp32 densities and posteriors, float64 statistics in a fixed order), the
               M-step on the host in float64
    speakers   MAP adaptation of the UBM's weights AND means to a speaker's enrolment frames (relevance 16), variances kept
    score      mean per-frame log-likelihood of an utterance under every model in one dvae_gmm_score launch; the
               log-likelihood ratio is a speaker's column minus the UBM's.  An utterance without voiced frames scores NaN,
               is listed and left out of every mean.

Deterministic: the same files give the same bits, whatever else shares a batch.  UNPINNED against any published
speaker-verification system: the figures compare runs of this project on one corpus.  GPU only, no CPU fallback.
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

from . import evaluate as ev
from ._lib import check, lib, ptr, stream
from .packed import upload
from .preprocess import read_wav

MAX_K = 256                   # DVAE_GMM_MAX_K
MAX_DIM = 32                  # DVAE_GMM_MAX_DIM
COL0 = 1                      # first coefficient used: c0 is dropped
FEATURE_DIM = ev.DIM - COL0   # 23
VAR_FLOOR = 0.01              # of the global per-dimension variance
WEIGHT_FLOOR = 1e-6
RELEVANCE = 16.0
LOG_2PI = math.log(2.0 * math.pi)
FEATURE_CONSTANTS = dict(sample_rate=ev.SAMPLE_RATE, hop=ev.HOP, frame=ev.FRAME, fft_size=ev.FFT_SIZE, order=ev.ORDER,
                         alpha=ev.ALPHA, col0=COL0, dim=FEATURE_DIM, voiced_peak=ev.VOICED_PEAK,
                         voiced_rel_power=ev.VOICED_REL_POWER, lag_min=ev.LAG_MIN, lag_max=ev.LAG_MAX)


# ------------------------------------------------------------------------------------------------------ host, float64
class DiagGMM:
    """A diagonal-covariance Gaussian mixture: w [K], mu [K, D], var [K, D], float64 numpy."""

    def __init__(self, w, mu, var):
        self.w = np.array(w, dtype=np.float64).reshape(-1)
        self.mu = np.array(mu, dtype=np.float64)
        self.var = np.array(var, dtype=np.float64)
        K = self.w.shape[0]
        if self.mu.ndim != 2 or self.mu.shape[0] != K or self.var.shape != self.mu.shape:
            raise ValueError(f"DiagGMM: w {self.w.shape}, mu {self.mu.shape}, var {self.var.shape}")
        if not 1 <= K <= MAX_K or not 1 <= self.mu.shape[1] <= MAX_DIM:
            raise ValueError(f"DiagGMM: K = {K}, D = {self.mu.shape[1]}; the kernels support K <= {MAX_K}, D <= {MAX_DIM}")
        if not (np.all(self.w > 0) and np.all(self.var > 0) and np.all(np.isfinite(self.mu))):
            raise ValueError("DiagGMM: weights and variances must be positive, means finite")

    @property
    def K(self) -> int:
        return self.w.shape[0]

    @property
    def D(self) -> int:
        return self.mu.shape[1]

    def tables(self):
        """the model on the device, computed in float64 and rounded once: a [K] = ln w - 1/2 sum_d ln(2 pi var), mu [K, D],
        prec [K, D] = 1 / var; fp32 numpy"""
        a = np.log(self.w) - 0.5 * np.sum(LOG_2PI + np.log(self.var), axis=1)
        return a.astype(np.float32), self.mu.astype(np.float32), (1.0 / self.var).astype(np.float32)

    def save(self, path) -> None:
        """.npz of the three arrays and the constants that define the features"""
        with open(path, "wb") as f:
            np.savez(f, w=self.w, mu=self.mu, var=self.var, **{k: np.asarray(v) for k, v in FEATURE_CONSTANTS.items()})

    @classmethod
    def load(cls, path) -> "DiagGMM":
        with np.load(path, allow_pickle=False) as z:
            for k, v in FEATURE_CONSTANTS.items():
                if k not in z.files or z[k].item() != v:
                    raise ValueError(f"{path}: fitted on other features ({k} = "
                                     f"{z[k].item() if k in z.files else 'missing'}, here {v})")
            return cls(z["w"], z["mu"], z["var"])


def stats_size(K: int, D: int) -> int:
    return K * (1 + 2 * D) + 1


def unpack_stats(stats, K: int, D: int):
    """dvae_gmm_estep's stats -> n [K], f [K, D], s [K, D], sum of lse"""
    v = np.asarray(stats, dtype=np.float64).reshape(-1)
    if v.shape[0] != stats_size(K, D):
        raise ValueError(f"stats: {v.shape[0]} values, expected {stats_size(K, D)} for K = {K}, D = {D}")
    rec = v[:-1].reshape(K, 1 + 2 * D)
    return rec[:, 0].copy(), rec[:, 1:1 + D].copy(), rec[:, 1 + D:].copy(), float(v[-1])


def init_indices(n_frames: int, K: int, seed: int) -> np.ndarray:
    """the K distinct frames the means start at"""
    if not 1 <= K <= n_frames:
        raise ValueError(f"{K} components need at least {K} frames, got {n_frames}")
    return np.random.default_rng(seed).choice(n_frames, size=K, replace=False)


def initial_model(frames, gvar) -> DiagGMM:
    """means = the drawn frames [K, D], every variance the global per-dimension variance, uniform weights"""
    frames = np.asarray(frames, dtype=np.float64)
    K = frames.shape[0]
    return DiagGMM(np.full(K, 1.0 / K), frames, np.tile(np.asarray(gvar, dtype=np.float64), (K, 1)))


def m_step(model: DiagGMM, stats, n_frames: int, gvar) -> DiagGMM:
    """w = n / N, mu = f / n, var = max(s / n - mu^2, VAR_FLOOR * gvar); a component with n_k < D + 1 keeps its mean and
    variance; weights are floored at WEIGHT_FLOOR and renormalised"""
    n, f, s, _ = unpack_stats(stats, model.K, model.D)
    ok = n >= model.D + 1
    nn = np.where(ok, n, 1.0)[:, None]
    mu = np.where(ok[:, None], f / nn, model.mu)
    var = np.where(ok[:, None], np.maximum(s / nn - mu * mu, VAR_FLOOR * np.asarray(gvar, dtype=np.float64)[None]),
                   model.var)
    w = np.maximum(n / n_frames, WEIGHT_FLOOR)
    return DiagGMM(w / w.sum(), mu, var)


def map_adapt(ubm: DiagGMM, stats, n_frames: int, relevance: float = RELEVANCE) -> DiagGMM:
    """MAP adaptation of weights AND means to the statistics of a speaker's `n_frames` frames under the UBM:
    alpha_k = n_k / (n_k + relevance), mu'_k = alpha_k f_k / n_k + (1 - alpha_k) mu_k, w'_k proportional to
    alpha_k n_k / T + (1 - alpha_k) w_k (scaled to the UBM's total weight); variances kept"""
    n, f, _, _ = unpack_stats(stats, ubm.K, ubm.D)
    if n_frames < 1 or relevance < 0:
        raise ValueError("map_adapt: needs frames and a relevance >= 0")
    with np.errstate(invalid="ignore", divide="ignore"):
        alpha = np.where(n > 0, n / (n + relevance), 0.0)
    mean = np.where(n[:, None] > 0, f / np.where(n > 0, n, 1.0)[:, None], ubm.mu)
    mu = alpha[:, None] * mean + (1.0 - alpha[:, None]) * ubm.mu
    w = alpha * n / n_frames + (1.0 - alpha) * ubm.w
    return DiagGMM(w * (ubm.w.sum() / w.sum()), mu, ubm.var)


def mean_scores(sums, counts) -> np.ndarray:
    """[n_utt, M] sums of per-frame log-likelihoods and [n_utt] frame counts -> means, NaN rows where count == 0"""
    sums, counts = np.asarray(sums, dtype=np.float64), np.asarray(counts).reshape(-1, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(counts > 0, sums / np.maximum(counts, 1), np.nan)


def finite_mean(v) -> float:
    v = np.asarray(v, dtype=np.float64)
    v = v[np.isfinite(v)]
    return float(v.mean()) if v.size else float("nan")


# ------------------------------------------------------------------------------------------------------------ GPU passes
def _device_tables(models: Sequence[DiagGMM], device):
    K, D = models[0].K, models[0].D
    if any(m.K != K or m.D != D for m in models):
        raise ValueError("every model of one launch has the same K and D")
    tabs = [m.tables() for m in models]
    return tuple(upload(np.stack([t[i] for t in tabs]), device) for i in range(3))


def estep(features, model: DiagGMM, col0: int = COL0, lse=None, gamma=None) -> np.ndarray:
    """one dvae_gmm_estep over all rows of the device buffer `features` [N, ld] (fp32, contiguous) -> stats, float64
    numpy [K (1 + 2 D) + 1].  lse [N] / gamma [N, K]: optional fp32 device buffers to fill."""
    if not (torch.is_tensor(features) and features.is_cuda and features.dtype == torch.float32 and features.dim() == 2
            and features.is_contiguous()):
        raise RuntimeError("estep: features must be a contiguous fp32 [N, ld] tensor on the GPU (no CPU fallback)")
    N, ld = int(features.shape[0]), int(features.shape[1])
    a, mu, prec = _device_tables([model], features.device)
    L = lib()
    ws = torch.empty(max(1, int(L.dvae_gmm_ws_bytes(N, model.K, model.D))), device=features.device, dtype=torch.uint8)
    stats = torch.empty(stats_size(model.K, model.D), device=features.device, dtype=torch.float64)
    check(L.dvae_gmm_estep(ptr(features), ld, col0, N, model.D, ptr(a), ptr(mu), ptr(prec), model.K, ptr(lse), ptr(gamma),
                           ptr(ws), ptr(stats), stream()), "dvae_gmm_estep")
    return stats.cpu().numpy()


def score_segments(features, segs, models: Sequence[DiagGMM], col0: int = COL0) -> np.ndarray:
    """one dvae_gmm_score launch: features [rows, ld] on the device, segs [nseg, 2] int64 {row0, count} (host) ->
    [nseg, len(models)] float64 sums of the per-frame log-likelihoods"""
    segs = np.ascontiguousarray(segs, dtype=np.int64).reshape(-1, 2)
    rows, ld = int(features.shape[0]), int(features.shape[1])
    if len(segs) and (segs.min() < 0 or (segs[:, 0] + segs[:, 1]).max() > rows):
        raise ValueError("score_segments: a segment leaves the feature buffer")
    a, mu, prec = _device_tables(models, features.device)
    out = torch.empty((len(segs), len(models)), device=features.device, dtype=torch.float64)
    check(lib().dvae_gmm_score(ptr(features), ld, col0, models[0].D, ptr(upload(segs, features.device, np.int64)),
                               len(segs), ptr(a), ptr(mu), ptr(prec), models[0].K, len(models), ptr(out), stream()),
          "dvae_gmm_score")
    return out.cpu().numpy()


def global_variance(features, col0: int = COL0, dim: int = FEATURE_DIM) -> np.ndarray:
    """per-dimension variance of all frames, from the kernel's own float64 sums: one component at mean 0 and variance 1
    has gamma = 1 on every frame, so its statistics are sum x and sum x^2"""
    N = int(features.shape[0])
    one = DiagGMM(np.ones(1), np.zeros((1, dim)), np.ones((1, dim)))
    _, f, s, _ = unpack_stats(estep(features, one, col0), 1, dim)
    return s[0] / N - (f[0] / N) ** 2


def train_ubm(features, K: int = 64, iters: int = 10, seed: int = 0, col0: int = COL0, dim: int = FEATURE_DIM, log=None,
              history: list = None):
    """EM on ONE packed device buffer `features` [N, ld]: frame t is features[t, col0:col0 + dim].  One dvae_gmm_estep call
    per iteration covers all N, so the result's bits do not depend on how the audio was batched.  -> (DiagGMM, [mean
    log-likelihood per frame of each iteration]).  log: called with (iteration, mean log-likelihood); history: a list
    that receives, per iteration, dict(model = the parameters its E-step ran on, stats, gvar)."""
    N = int(features.shape[0])
    idx = init_indices(N, K, seed)
    gvar = global_variance(features, col0, dim)
    if not np.all(gvar > 0):
        raise ValueError("train_ubm: a feature dimension has no variance")
    frames = features[torch.from_numpy(idx).to(features.device)][:, col0:col0 + dim].cpu().numpy()
    model = initial_model(frames, gvar)
    lls = []
    for i in range(iters):
        stats = estep(features, model, col0)
        lls.append(float(stats[-1]) / N)
        if log is not None:
            log(i, lls[-1])
        if history is not None:
            history.append(dict(model=model, stats=stats, gvar=gvar))
        model = m_step(model, stats, N, gvar)
    return model, lls


def voiced_rows(table, count) -> np.ndarray:
    """row indices of every utterance's voiced frames in the feats buffer of MelCepstrum.packed, in utterance order"""
    return np.concatenate([np.arange(r0, r0 + k, dtype=np.int64) for r0, k in zip(table[:, 0], count)] +
                          [np.zeros(0, dtype=np.int64)])


def gather_voiced(out: dict):
    """MelCepstrum.packed's result -> its voiced frames back to back, [sum count, 24] on the device"""
    rows = voiced_rows(out["table"], out["count"])
    return out["feats"][torch.from_numpy(rows).to(out["feats"].device)].contiguous()


class Verifier:
    """Speaker models MAP-adapted from `ubm`, and the scores of utterances under all of them."""

    def __init__(self, ubm: DiagGMM, device="cuda", relevance: float = RELEVANCE, batch: int = 32):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("Verifier runs on the HIP path only (no CPU fallback)")
        self.ubm, self.relevance, self.batch = ubm, float(relevance), int(batch)
        self.speakers, self.models = [], []
        self._features = None

    @property
    def features(self) -> ev.MelCepstrum:
        """the feature pass of the audio entry points (enroll, score, llr); the *_frames ones take any dimension"""
        if self.ubm.D != FEATURE_DIM:
            raise ValueError(f"the UBM has {self.ubm.D} dimensions, the mel-cepstral features {FEATURE_DIM}")
        if self._features is None:
            self._features = ev.MelCepstrum(self.device)
        return self._features

    def adapt(self, frames, col0: int = COL0) -> DiagGMM:
        """the UBM adapted to the frames of a device buffer [n, ld]"""
        return map_adapt(self.ubm, estep(frames, self.ubm, col0), int(frames.shape[0]), self.relevance)

    def enroll(self, speakers: dict, srs: dict = None) -> None:
        """{speaker: [waveforms]} (srs: {speaker: [sample rates]}, default 16 kHz): one model per speaker"""
        for name, wavs in speakers.items():
            rates = None if srs is None else srs.get(name)
            parts = []
            for i in range(0, len(wavs), self.batch):
                parts.append(gather_voiced(self.features.packed(list(wavs[i:i + self.batch]),
                                                                None if rates is None else rates[i:i + self.batch])))
            frames = torch.cat(parts) if parts else None
            if frames is None or frames.shape[0] == 0:
                raise ValueError(f"speaker {name}: no voiced frame to enrol from")
            model = self.adapt(frames)
            if name in self.speakers:
                self.models[self.speakers.index(name)] = model
            else:
                self.speakers.append(name)
                self.models.append(model)

    def enroll_frames(self, speakers: dict, col0: int = COL0) -> None:
        """{speaker: device buffer [n, ld] of frames}: the same, from features"""
        for name, frames in speakers.items():
            self.speakers.append(name)
            self.models.append(self.adapt(frames, col0))

    def score_frames(self, features, segs, col0: int = COL0) -> np.ndarray:
        """[nseg, 1 + n_speakers] mean per-frame log-likelihoods of the segments {row0, count} of a device buffer"""
        segs = np.asarray(segs, dtype=np.int64).reshape(-1, 2)
        return mean_scores(score_segments(features, segs, [self.ubm] + self.models, col0), segs[:, 1])

    def score(self, wavs: Sequence, srs: Sequence[int] = None) -> np.ndarray:
        """float64 [n_utt, 1 + n_speakers] mean per-frame log-likelihoods, column 0 the UBM's; NaN rows for utterances
        without voiced frames.  All models in one dvae_gmm_score launch per packed batch."""
        res = []
        for i in range(0, len(wavs), self.batch):
            out = self.features.packed(list(wavs[i:i + self.batch]), None if srs is None else list(srs[i:i + self.batch]))
            res.append(self.score_frames(out["feats"], np.stack([out["table"][:, 0], out["count"]], axis=1)))
        return np.concatenate(res) if res else np.zeros((0, 1 + len(self.models)))

    def llr(self, wavs: Sequence, srs: Sequence[int] = None) -> np.ndarray:
        """[n_utt, n_speakers]: the speakers' columns minus the UBM's"""
        s = self.score(wavs, srs)
        return s[:, 1:] - s[:, :1]


# ------------------------------------------------------------------------------------------------------------------ CLI
def corpus_files(root: Path, max_utts: int) -> dict:
    """{speaker: the first max_utts of <root>/<speaker>/**/*.wav in sorted order}, speakers sorted"""
    out = {}
    for d in sorted(p for p in Path(root).iterdir() if p.is_dir()):
        files = sorted(d.rglob("*.wav"), key=str)[:max_utts]
        if files:
            out[d.name] = files
    return out


def split_enrolment(files: Sequence, enroll_utts: int):
    """sorted files -> (the first enroll_utts, the rest)"""
    files = sorted(files, key=str)
    return files[:enroll_utts], files[enroll_utts:]


def decide(llr_own, llr_other) -> dict:
    """the threshold-free two-way identification over files: a file counts for its own speaker when llr_own > llr_other;
    files with a NaN (no voiced frames) are listed and left out.  -> dict(hits, scored, unvoiced [indices], flags)"""
    own, other = np.asarray(llr_own, dtype=np.float64), np.asarray(llr_other, dtype=np.float64)
    fin = np.isfinite(own) & np.isfinite(other)
    flags = [bool(a > b) if ok else None for a, b, ok in zip(own, other, fin)]
    return dict(hits=int(sum(1 for f in flags if f)), scored=int(fin.sum()), unvoiced=[int(i) for i in np.nonzero(~fin)[0]],
                flags=flags)


def _parse(argv):
    p = argparse.ArgumentParser(prog="python -m dvae_amd.verify",
                                description="GMM-UBM speaker verification of converted .wav files, on the GPU.")
    sub = p.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("train", help="fit the universal background model on a corpus of 16 kHz wavs")
    t.add_argument("wav16_root", type=Path, help="<root>/<speaker>/**/*.wav")
    t.add_argument("-o", "--out", type=Path, required=True, help="the UBM's .npz")
    t.add_argument("--components", type=int, default=64)
    t.add_argument("--iters", type=int, default=10)
    t.add_argument("--max-utts-per-speaker", type=int, default=40)
    t.add_argument("--seed", type=int, default=0)
    s = sub.add_parser("score", help="score converted wavs against a target and a source speaker")
    s.add_argument("converted_dir", type=Path)
    s.add_argument("--ubm", type=Path, required=True)
    s.add_argument("--target", type=Path, required=True, help="directory of the target speaker's natural wavs")
    s.add_argument("--source", type=Path, required=True, help="directory of the source speaker's natural wavs")
    s.add_argument("--enroll-utts", type=int, default=20)
    s.add_argument("--relevance", type=float, default=RELEVANCE)
    s.add_argument("--json", type=Path, default=None, help="default <converted_dir>/verify.json")
    args = p.parse_args(argv)
    if args.cmd == "train" and (not 1 <= args.components <= MAX_K or args.iters < 1 or args.max_utts_per_speaker < 1):
        p.error(f"train: 1 <= --components <= {MAX_K}, --iters >= 1, --max-utts-per-speaker >= 1")
    if args.cmd == "score" and (args.enroll_utts < 1 or args.relevance < 0):
        p.error("score: --enroll-utts >= 1, --relevance >= 0")
    return args


def _read(files):
    wavs, srs = [], []
    for f in files:
        w, sr = read_wav(f)
        wavs.append(w)
        srs.append(sr)
    return wavs, srs


def _train(args) -> int:
    if not args.wav16_root.is_dir():
        print(f"verify: {args.wav16_root} is not a directory", file=sys.stderr)
        return 2
    corpus = corpus_files(args.wav16_root, args.max_utts_per_speaker)
    files = [f for fs in corpus.values() for f in fs]
    if not files:
        print(f"verify: no <speaker>/**/*.wav under {args.wav16_root}", file=sys.stderr)
        return 1
    fe, parts, batch = ev.MelCepstrum(), [], 32
    for i in range(0, len(files), batch):
        wavs, srs = _read(files[i:i + batch])
        parts.append(gather_voiced(fe.packed(wavs, srs)))
    features = torch.cat(parts).contiguous()
    print(f"{len(corpus)} speakers, {len(files)} files, {features.shape[0]} voiced frames")
    if features.shape[0] < args.components:
        print(f"verify: {features.shape[0]} voiced frames for {args.components} components", file=sys.stderr)
        return 1
    model, lls = train_ubm(features, args.components, args.iters, args.seed,
                           log=lambda i, ll: print(f"iteration {i}: mean log-likelihood {ll}"))
    model.save(args.out)
    print(f"wrote {args.out}: {model.K} components, {model.D} dimensions")
    return 0


def _score(args) -> int:
    for d in (args.converted_dir, args.target, args.source):
        if not d.is_dir():
            print(f"verify: {d} is not a directory", file=sys.stderr)
            return 2
    ubm = DiagGMM.load(args.ubm)
    converted = sorted(args.converted_dir.glob("*.wav"), key=str)
    enrol_t, rest_t = split_enrolment(args.target.glob("*.wav"), args.enroll_utts)
    enrol_s, rest_s = split_enrolment(args.source.glob("*.wav"), args.enroll_utts)
    if not converted or not enrol_t or not enrol_s:
        print("verify: needs *.wav files in the converted, the target and the source directory", file=sys.stderr)
        return 1
    v = Verifier(ubm, relevance=args.relevance)
    (wt, rt), (ws_, rs_) = _read(enrol_t), _read(enrol_s)
    v.enroll(dict(target=wt, source=ws_), dict(target=rt, source=rs_))
    num = lambda x: float(x) if math.isfinite(float(x)) else None

    def rows(files, own):
        """per-file llr rows and the decision for column `own` (0 target, 1 source)"""
        if not files:
            return [], decide([], [])
        llr = v.llr(*_read(files))
        d = decide(llr[:, own], llr[:, 1 - own])
        return [dict(utterance=ev.utterance_id(f), file=str(f), llr_target=num(a), llr_source=num(b), accepted=flag)
                for f, (a, b), flag in zip(files, llr, d["flags"])], d

    conv, dc = rows(converted, 0)
    for r in conv:
        if r["accepted"] is None:
            print(f"utterance {r['utterance']} llr: nan (no voiced frames)")
        else:
            print(f"utterance {r['utterance']} llr: target {r['llr_target']} source {r['llr_source']}")
    mt = finite_mean([r["llr_target"] for r in conv if r["accepted"] is not None])
    ms = finite_mean([r["llr_source"] for r in conv if r["accepted"] is not None])
    print(f"target accepted: {dc['hits']}/{dc['scored']}")
    print(f"mean llr: target {mt} source {ms} over {dc['scored']} of {len(conv)} files")
    nat_t, dt = rows(rest_t, 0)
    nat_s, ds = rows(rest_s, 1)
    nat_hits, nat_scored = dt["hits"] + ds["hits"], dt["scored"] + ds["scored"]
    print(f"natural speech identified: {nat_hits}/{nat_scored}")
    result = dict(converted_dir=str(args.converted_dir), target=str(args.target), source=str(args.source),
                  ubm=str(args.ubm), components=ubm.K, relevance=args.relevance, enroll_utts=args.enroll_utts,
                  enrolled=dict(target=[str(f) for f in enrol_t], source=[str(f) for f in enrol_s]),
                  files=conv, accepted=dc["hits"], scored=dc["scored"], mean_llr_target=num(mt), mean_llr_source=num(ms),
                  no_voiced=[conv[i]["file"] for i in dc["unvoiced"]],
                  natural=dict(identified=nat_hits, scored=nat_scored, target=nat_t, source=nat_s,
                               no_voiced=[nat_t[i]["file"] for i in dt["unvoiced"]] +
                                         [nat_s[i]["file"] for i in ds["unvoiced"]]))
    (args.json or args.converted_dir.joinpath("verify.json")).write_text(json.dumps(result, indent=1) + "\n")
    return 0


def main(argv=None) -> int:
    args = _parse(sys.argv[1:] if argv is None else argv)
    return _train(args) if args.cmd == "train" else _score(args)


if __name__ == "__main__":
    sys.exit(main())
