"""i-vector speaker embeddings on the GPU: cosine similarity between a conversion and its target SPEAKER,
and the equal error rate of the speaker instruments on the user's own corpus.

    python -m dvae_amd.ivector train <wav16_root> --ubm ubm.npz -o ivec.npz [--rank 32] [--iters 10]
           [--max-utts-per-speaker 40] [--seed 0] [--no-min-divergence]
    python -m dvae_amd.ivector score <converted_dir> --ubm ubm.npz --ivector ivec.npz --target <wav dir> --source <wav dir>
           [--enroll-utts 20] [--json PATH]
    python -m dvae_amd.ivector eer <wav16_root> --ubm ubm.npz --ivector ivec.npz [--enroll-utts 20]
           [--max-utts-per-speaker 40] [--json PATH]

The classical embedding (Dehak et al. 2011; Kenny 2005, 2008), no second network and no pretrained weights, on top of the
UBM of `verify` (§4.13) and its features:

    statistics  per utterance, under the UBM: n_c = sum_t gamma_tc, f_cd = (sum_t gamma_tc x_td - n_c mu_cd) sqrt(prec_cd)
                (dvae_gmm_utt_stats: the E-step's fp32 posteriors, float64 sums in a fixed order)
    model       the supervector of an utterance is T w, w ~ N(0, I): T [K D, R] in the whitened space
    posterior   L = I + sum_c n_c T_c^T T_c, w = L^-1 T^T f, S = L^-1 + w w^T (dvae_ivec_posterior: one utterance per
                workgroup, Cholesky and both substitutions on chip, float64); w is the i-vector
    training    EM with fixed alignments: dvae_ivec_accumulate sums n S, f w^T and S over the utterances, the M-step
                T_c = C_c A_c^-1 and the minimum-divergence step T <- T chol(sum S / U) run on the host in float64
    backend     mean subtraction, whitening by the training i-vectors' total covariance, length normalisation
                (Garcia-Romero & Espy-Wilson 2011); a speaker is the length-normalised mean of its enrolment utterances'
                normalised i-vectors; a score is the cosine

An utterance without voiced frames gives a NaN row, is listed and left out of every mean.  Deterministic: the same files
give the same bits.  NOT here: PLDA, LDA / WCCN, score normalisation, re-estimation of the UBM's covariances, i-vectors in
`latent_map`.  UNPINNED against any published system.  GPU only, no CPU fallback.
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
from . import verify
from ._lib import check, lib, ptr, stream
from .packed import upload
from .verify import COL0, FEATURE_CONSTANTS, DiagGMM

MAX_R = 64               # DVAE_IVEC_MAX_R
N_FLOOR = 1e-3           # a component whose sum_u n_uc is below it keeps its rows of T in the M-step (a setting)
INIT_SCALE = 0.1         # the initial T is standard normal times this (a setting, not a measured optimum)
EIG_FLOOR = 1e-10        # the backend's eigenvalues are floored at this times the largest
SYMBOLS = ("dvae_gmm_utt_stats", "dvae_ivec_posterior", "dvae_ivec_ws_bytes", "dvae_ivec_accumulate")


def _lib():
    L = lib()
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    if missing:
        raise RuntimeError(f"the loaded library lacks {', '.join(missing)}: stale build — rebuild the library with "
                           "`python -c 'import __graft_entry__ as g; g.build()'`")
    return L


def _dev64(t, shape, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape):
        raise RuntimeError(f"{what}: a contiguous float64 {list(shape)} tensor on the GPU is needed (no CPU fallback)")
    return t


# -------------------------------------------------------------------------------------------------------- host, float64
def gram(T, dim: int) -> np.ndarray:
    """T [K dim, R] -> P [K, R, R], P_c = T_c^T T_c, float64 on the host (the kernels read j <= i)"""
    T = np.asarray(T, dtype=np.float64)
    if T.ndim != 2 or dim < 1 or T.shape[0] % dim:
        raise ValueError(f"gram: T {T.shape} is not [K * {dim}, R]")
    Tc = T.reshape(T.shape[0] // dim, dim, T.shape[1])
    return np.einsum("cdi,cdj->cij", Tc, Tc)


def initial_T(K: int, D: int, rank: int, seed: int, scale: float = INIT_SCALE) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal((K * D, rank)) * scale


def m_step(T, A, C, nsum, D: int, n_floor: float = N_FLOOR) -> np.ndarray:
    """T_c = C_c A_c^-1 by numpy.linalg.solve (T_c A_c = C_c); a component with nsum_c < n_floor keeps its rows"""
    T = np.array(T, dtype=np.float64)
    for c in range(len(nsum)):
        if nsum[c] >= n_floor:
            T[c * D:(c + 1) * D] = np.linalg.solve(A[c].T, C[c * D:(c + 1) * D].T).T
    return T


def apply_min_divergence(T, Ssum, U: int) -> np.ndarray:
    """T chol(Ssum / U): the factor's second moment over the training utterances becomes the identity"""
    return np.asarray(T, dtype=np.float64) @ np.linalg.cholesky(np.asarray(Ssum, dtype=np.float64) / U)


class Backend:
    """mean subtraction, whitening by the total covariance, length normalisation; float64 on the host"""

    def __init__(self, mean, W):
        self.mean, self.W = np.array(mean, dtype=np.float64), np.array(W, dtype=np.float64)

    @classmethod
    def fit(cls, w, eig_floor: float = EIG_FLOOR) -> "Backend":
        w = np.asarray(w, dtype=np.float64)
        w = w[np.isfinite(w).all(axis=1)]
        if len(w) < 1:
            raise ValueError("Backend.fit: no finite i-vector")
        mean = w.mean(axis=0)
        c = w - mean
        lam, V = np.linalg.eigh(c.T @ c / len(w))
        lam = np.maximum(lam, eig_floor * max(lam.max(), np.finfo(np.float64).tiny))
        return cls(mean, V / np.sqrt(lam)[None])

    def transform(self, w) -> np.ndarray:
        """[..., R] -> unit vectors (NaN rows stay NaN)"""
        y = (np.asarray(w, dtype=np.float64) - self.mean) @ self.W
        return y / np.maximum(np.linalg.norm(y, axis=-1, keepdims=True), np.finfo(np.float64).tiny)

    @staticmethod
    def speaker(ws) -> np.ndarray:
        """normalised i-vectors of the enrolment utterances [n, R] (NaN rows left out) -> the speaker's unit vector"""
        ws = np.asarray(ws, dtype=np.float64).reshape(-1, np.shape(ws)[-1])
        ws = ws[np.isfinite(ws).all(axis=1)]
        if len(ws) < 1:
            raise ValueError("Backend.speaker: no utterance with voiced frames to enrol from")
        m = ws.mean(axis=0)
        return m / max(np.linalg.norm(m), np.finfo(np.float64).tiny)


def cosine_scores(utts, speakers) -> np.ndarray:
    """[n, R] x [m, R] -> [n, m] cosines (NaN rows for NaN utterances)"""
    a, b = np.asarray(utts, dtype=np.float64), np.asarray(speakers, dtype=np.float64)
    den = np.linalg.norm(a, axis=1)[:, None] * np.linalg.norm(b, axis=1)[None]
    with np.errstate(invalid="ignore"):
        return (a @ b.T) / np.maximum(den, np.finfo(np.float64).tiny)


def eer(target_scores, nontarget_scores):
    """-> (equal error rate, threshold).  Operating point k accepts a score >= t_k, t_k the distinct scores ascending, and a
    last point accepts nothing; false-accept rate falls and false-reject rate rises along them, and the result is where the
    two cross, linearly interpolated between the two adjacent points.  NaNs and empty lists are refused."""
    tar = np.sort(np.asarray(target_scores, dtype=np.float64).reshape(-1))
    non = np.sort(np.asarray(nontarget_scores, dtype=np.float64).reshape(-1))
    if tar.size == 0 or non.size == 0 or np.isnan(tar).any() or np.isnan(non).any():
        raise ValueError("eer: needs target and non-target scores, none of them NaN")
    thr = np.unique(np.concatenate([tar, non]))
    frr = np.concatenate([np.searchsorted(tar, thr, side="left"), [tar.size]]) / tar.size
    far = np.concatenate([non.size - np.searchsorted(non, thr, side="left"), [0]]) / non.size
    thr = np.concatenate([thr, thr[-1:]])
    d = frr - far
    i = int(np.nonzero(d >= 0)[0][0])
    if i == 0 or d[i] == 0:
        return float(frr[i]), float(thr[i])
    s = -d[i - 1] / (d[i] - d[i - 1])
    return float(frr[i - 1] + s * (frr[i] - frr[i - 1])), float(thr[i - 1] + s * (thr[i] - thr[i - 1]))


# ------------------------------------------------------------------------------------------------------------ GPU passes
def utterance_stats(features, segs, ubm: DiagGMM, col0: int = COL0):
    """one dvae_gmm_utt_stats launch: features [rows, ld] fp32 on the device, segs [U, 2] int64 {row0, count} (host) ->
    (n [U, K], f [U, K D]) float64 device tensors; a segment without frames gives zeros"""
    if not (torch.is_tensor(features) and features.is_cuda and features.dtype == torch.float32 and features.dim() == 2
            and features.is_contiguous()):
        raise RuntimeError("utterance_stats: features must be a contiguous fp32 [rows, ld] tensor on the GPU (no CPU fallback)")
    segs = np.ascontiguousarray(segs, dtype=np.int64).reshape(-1, 2)
    rows, ld = int(features.shape[0]), int(features.shape[1])
    if len(segs) < 1 or segs.min() < 0 or (segs[:, 0] + segs[:, 1]).max() > rows:
        raise ValueError("utterance_stats: needs segments, all inside the feature buffer")
    a, mu, prec = (upload(t, features.device) for t in ubm.tables())
    n = torch.empty((len(segs), ubm.K), device=features.device, dtype=torch.float64)
    f = torch.empty((len(segs), ubm.K * ubm.D), device=features.device, dtype=torch.float64)
    check(_lib().dvae_gmm_utt_stats(ptr(features), ld, col0, ubm.D, ptr(upload(segs, features.device, np.int64)), len(segs),
                                    ptr(a), ptr(mu), ptr(prec), ubm.K, ptr(n), ptr(f), stream()), "dvae_gmm_utt_stats")
    return n, f


def posterior(n, f, T, P, want_S: bool = False, want_ll: bool = False):
    """one dvae_ivec_posterior launch on device float64 tensors n [U, K], f [U, K D], T [K D, R], P [K, R, R] ->
    (w [U, R], S [U, R, R] or None, ll [U] or None)"""
    U, K, R = int(n.shape[0]), int(n.shape[1]), int(T.shape[1])
    D = int(T.shape[0]) // K
    _dev64(n, (U, K), "n"), _dev64(f, (U, K * D), "f"), _dev64(T, (K * D, R), "T"), _dev64(P, (K, R, R), "P")
    w = torch.empty((U, R), device=n.device, dtype=torch.float64)
    S = torch.empty((U, R, R), device=n.device, dtype=torch.float64) if want_S else None
    ll = torch.empty((U,), device=n.device, dtype=torch.float64) if want_ll else None
    check(_lib().dvae_ivec_posterior(ptr(n), ptr(f), ptr(T), ptr(P), U, K, D, R, ptr(w), ptr(S), ptr(ll), stream()),
          "dvae_ivec_posterior")
    return w, S, ll


def accumulate(n, f, w, S):
    """one dvae_ivec_accumulate call -> (A [K, R, R], C [K D, R], Ssum [R, R]) float64 numpy"""
    U, K, R = int(n.shape[0]), int(n.shape[1]), int(w.shape[1])
    D = int(f.shape[1]) // K
    L = _lib()
    ws = torch.empty(max(1, int(L.dvae_ivec_ws_bytes(U, K, D, R))), device=n.device, dtype=torch.uint8)
    A = torch.empty((K, R, R), device=n.device, dtype=torch.float64)
    C = torch.empty((K * D, R), device=n.device, dtype=torch.float64)
    Ssum = torch.empty((R, R), device=n.device, dtype=torch.float64)
    check(L.dvae_ivec_accumulate(ptr(n), ptr(f), ptr(w), ptr(S), U, K, D, R, ptr(ws), ptr(A), ptr(C), ptr(Ssum), stream()),
          "dvae_ivec_accumulate")
    return A.cpu().numpy(), C.cpu().numpy(), Ssum.cpu().numpy()


def train_extractor(n, f, rank: int, iters: int = 10, seed: int = 0, min_divergence: bool = True, batch: int = 4096,
                    log=None, history: list = None, n_floor: float = N_FLOOR, init_scale: float = INIT_SCALE):
    """EM of the total-variability matrix on device statistics n [U, K], f [U, K D] (float64).  The utterances go through
    dvae_ivec_posterior / dvae_ivec_accumulate in chunks of `batch`, and the chunks' accumulators are added on the host in
    chunk order: `batch` is part of the configuration.  -> (T [K D, rank] numpy, [sum_u ll_u / U of each iteration]).
    log: called with (iteration, mean bound); history: a list that receives, per iteration, dict(T = the matrix its
    posteriors ran on, A, C, Ssum, ll)."""
    U, K = int(n.shape[0]), int(n.shape[1])
    D = int(f.shape[1]) // K
    if not (1 <= rank <= MAX_R) or iters < 1 or batch < 1 or U < 1 or D * K != int(f.shape[1]):
        raise ValueError(f"train_extractor: 1 <= rank <= {MAX_R}, iters >= 1, batch >= 1, f [U, K D]")
    _dev64(n, (U, K), "n"), _dev64(f, (U, K * D), "f")
    nsum = n.sum(dim=0).cpu().numpy()
    T, lls = initial_T(K, D, rank, seed, init_scale), []
    for it in range(iters):
        Td, Pd = upload(T, n.device, np.float64), upload(gram(T, D), n.device, np.float64)
        A, C, Ssum, ll = 0.0, 0.0, 0.0, 0.0
        for i in range(0, U, batch):
            nb, fb = n[i:i + batch], f[i:i + batch]
            w, S, l = posterior(nb, fb, Td, Pd, True, True)
            a, c, s = accumulate(nb, fb, w, S)
            A, C, Ssum, ll = A + a, C + c, Ssum + s, ll + float(l.cpu().numpy().sum())
        lls.append(ll / U)
        if log is not None:
            log(it, lls[-1])
        if history is not None:
            history.append(dict(T=T, A=A, C=C, Ssum=Ssum, ll=ll))
        T = m_step(T, A, C, nsum, D, n_floor)
        if min_divergence:
            T = apply_min_divergence(T, Ssum, U)
    return T, lls


class Extractor:
    """i-vectors of utterances under a UBM and a trained T; `backend` turns them into unit vectors"""

    def __init__(self, ubm: DiagGMM, T, backend: Backend = None, device="cuda", config: dict = None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("Extractor runs on the HIP path only (no CPU fallback)")
        self.ubm, self.T, self.backend = ubm, np.array(T, dtype=np.float64), backend
        self.config = dict(config or {})
        if self.T.ndim != 2 or self.T.shape[0] != ubm.K * ubm.D or not 1 <= self.T.shape[1] <= MAX_R:
            raise ValueError(f"Extractor: T {self.T.shape} for a UBM of K = {ubm.K}, D = {ubm.D} (rank <= {MAX_R})")
        self._Td = self._Pd = self._features = None
        self.batch = 32

    @property
    def rank(self) -> int:
        return self.T.shape[1]

    def _tables(self):
        if self._Td is None:
            self._Td = upload(self.T, self.device, np.float64)
            self._Pd = upload(gram(self.T, self.ubm.D), self.device, np.float64)
        return self._Td, self._Pd

    def posterior(self, n, f, want_S: bool = False, want_ll: bool = False):
        return posterior(n, f, *self._tables(), want_S, want_ll)

    def extract_frames(self, features, segs, col0: int = COL0) -> np.ndarray:
        """[U, R] float64 i-vectors of the segments {row0, count} of a device feature buffer; NaN rows for count = 0"""
        segs = np.asarray(segs, dtype=np.int64).reshape(-1, 2)
        n, f = utterance_stats(features, segs, self.ubm, col0)
        w = self.posterior(n, f)[0].cpu().numpy()
        w[segs[:, 1] <= 0] = np.nan
        return w

    def extract(self, wavs: Sequence, srs: Sequence[int] = None) -> np.ndarray:
        """[n_utt, R] float64 i-vectors; NaN rows for utterances without voiced frames"""
        if self.ubm.D != verify.FEATURE_DIM:
            raise ValueError(f"the UBM has {self.ubm.D} dimensions, the mel-cepstral features {verify.FEATURE_DIM}")
        if self._features is None:
            self._features = ev.MelCepstrum(self.device)
        res = []
        for i in range(0, len(wavs), self.batch):
            out = self._features.packed(list(wavs[i:i + self.batch]), None if srs is None else list(srs[i:i + self.batch]))
            res.append(self.extract_frames(out["feats"], np.stack([out["table"][:, 0], out["count"]], axis=1)))
        return np.concatenate(res) if res else np.zeros((0, self.rank))

    def embed(self, wavs: Sequence, srs: Sequence[int] = None) -> np.ndarray:
        """the backend's unit vectors of `extract`"""
        if self.backend is None:
            raise ValueError("Extractor.embed: no backend")
        return self.backend.transform(self.extract(wavs, srs))

    def save(self, path) -> None:
        """.npz: T, the UBM's arrays, the backend, the constants that define the features and the training configuration"""
        arrays = dict(T=self.T, ubm_w=self.ubm.w, ubm_mu=self.ubm.mu, ubm_var=self.ubm.var)
        if self.backend is not None:
            arrays.update(backend_mean=self.backend.mean, backend_W=self.backend.W)
        arrays.update({k: np.asarray(v) for k, v in FEATURE_CONSTANTS.items()})
        arrays.update({"config_" + k: np.asarray(v) for k, v in sorted(self.config.items())})
        with open(path, "wb") as fh:
            np.savez(fh, **arrays)

    @classmethod
    def load(cls, path, ubm: DiagGMM = None, device="cuda") -> "Extractor":
        """ubm: the UBM the caller is going to use; one that differs from the extractor's own is a ValueError"""
        with np.load(path, allow_pickle=False) as z:
            for k, v in FEATURE_CONSTANTS.items():
                if k not in z.files or z[k].item() != v:
                    raise ValueError(f"{path}: fitted on other features ({k} = "
                                     f"{z[k].item() if k in z.files else 'missing'}, here {v})")
            own = DiagGMM(z["ubm_w"], z["ubm_mu"], z["ubm_var"])
            if ubm is not None and not (ubm.w.shape == own.w.shape and ubm.mu.shape == own.mu.shape and
                                        np.array_equal(ubm.w, own.w) and np.array_equal(ubm.mu, own.mu) and
                                        np.array_equal(ubm.var, own.var)):
                raise ValueError(f"{path}: trained on another UBM than the one given")
            backend = Backend(z["backend_mean"], z["backend_W"]) if "backend_mean" in z.files else None
            config = {k[len("config_"):]: z[k].item() for k in z.files if k.startswith("config_")}
            return cls(own, z["T"], backend, device, config)


# ------------------------------------------------------------------------------------------------------------------ CLI
def _parse(argv):
    p = argparse.ArgumentParser(prog="python -m dvae_amd.ivector",
                                description="i-vector speaker embeddings: cosine similarity and EER, on the GPU.")
    sub = p.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("train", help="fit the total-variability matrix and the backend on a corpus of 16 kHz wavs")
    t.add_argument("wav16_root", type=Path, help="<root>/<speaker>/**/*.wav")
    t.add_argument("--ubm", type=Path, required=True)
    t.add_argument("-o", "--out", type=Path, required=True, help="the extractor's .npz")
    t.add_argument("--rank", type=int, default=32)
    t.add_argument("--iters", type=int, default=10)
    t.add_argument("--max-utts-per-speaker", type=int, default=40)
    t.add_argument("--seed", type=int, default=0)
    t.add_argument("--no-min-divergence", action="store_true")
    s = sub.add_parser("score", help="cosine of converted wavs to a target and a source speaker")
    s.add_argument("converted_dir", type=Path)
    s.add_argument("--ubm", type=Path, required=True)
    s.add_argument("--ivector", type=Path, required=True)
    s.add_argument("--target", type=Path, required=True, help="directory of the target speaker's natural wavs")
    s.add_argument("--source", type=Path, required=True, help="directory of the source speaker's natural wavs")
    s.add_argument("--enroll-utts", type=int, default=20)
    s.add_argument("--json", type=Path, default=None, help="default <converted_dir>/ivector.json")
    e = sub.add_parser("eer", help="equal error rate of the cosine and of verify's log-likelihood ratio on a corpus")
    e.add_argument("wav16_root", type=Path, help="<root>/<speaker>/**/*.wav")
    e.add_argument("--ubm", type=Path, required=True)
    e.add_argument("--ivector", type=Path, required=True)
    e.add_argument("--enroll-utts", type=int, default=20)
    e.add_argument("--max-utts-per-speaker", type=int, default=40)
    e.add_argument("--json", type=Path, default=None)
    args = p.parse_args(argv)
    if args.cmd == "train" and (not 1 <= args.rank <= MAX_R or args.iters < 1 or args.max_utts_per_speaker < 1):
        p.error(f"train: 1 <= --rank <= {MAX_R}, --iters >= 1, --max-utts-per-speaker >= 1")
    if args.cmd == "score" and args.enroll_utts < 1:
        p.error("score: --enroll-utts >= 1")
    if args.cmd == "eer" and (args.enroll_utts < 1 or args.max_utts_per_speaker <= args.enroll_utts):
        p.error("eer: --enroll-utts >= 1 and --max-utts-per-speaker above it")
    return args


def _num(x):
    return float(x) if math.isfinite(float(x)) else None


def _train(args) -> int:
    if not args.wav16_root.is_dir():
        print(f"ivector: {args.wav16_root} is not a directory", file=sys.stderr)
        return 2
    ubm = DiagGMM.load(args.ubm)
    corpus = verify.corpus_files(args.wav16_root, args.max_utts_per_speaker)
    files = [f for fs in corpus.values() for f in fs]
    if not files:
        print(f"ivector: no <speaker>/**/*.wav under {args.wav16_root}", file=sys.stderr)
        return 1
    fe, ns, fs_, batch = ev.MelCepstrum(), [], [], 32
    for i in range(0, len(files), batch):
        out = fe.packed(*verify._read(files[i:i + batch]))
        keep = out["count"] > 0
        if keep.any():
            n, f = utterance_stats(out["feats"], np.stack([out["table"][:, 0], out["count"]], axis=1)[keep], ubm)
            ns.append(n)
            fs_.append(f)
    U = sum(int(n.shape[0]) for n in ns)
    print(f"{len(corpus)} speakers, {U} utterances ({len(files) - U} without voiced frames left out)")
    if U < 2:
        print("ivector: needs at least two utterances with voiced frames", file=sys.stderr)
        return 1
    n, f = torch.cat(ns).contiguous(), torch.cat(fs_).contiguous()
    config = dict(rank=args.rank, iters=args.iters, seed=args.seed, min_divergence=not args.no_min_divergence, batch=4096,
                  n_floor=N_FLOOR, init_scale=INIT_SCALE, eig_floor=EIG_FLOOR, utterances=U)
    T, _ = train_extractor(n, f, args.rank, args.iters, args.seed, config["min_divergence"], config["batch"],
                           log=lambda i, ll: print(f"iteration {i}: mean log-likelihood bound {ll}"))
    ex = Extractor(ubm, T, config=config)
    ex.backend = Backend.fit(ex.posterior(n, f)[0].cpu().numpy())
    ex.save(args.out)
    print(f"wrote {args.out}: rank {ex.rank}, {ubm.K} components, {ubm.D} dimensions")
    return 0


def _score(args) -> int:
    for d in (args.converted_dir, args.target, args.source):
        if not d.is_dir():
            print(f"ivector: {d} is not a directory", file=sys.stderr)
            return 2
    ubm = DiagGMM.load(args.ubm)
    ex = Extractor.load(args.ivector, ubm)
    if ex.backend is None:
        print(f"ivector: {args.ivector} holds no backend", file=sys.stderr)
        return 1
    converted = sorted(args.converted_dir.glob("*.wav"), key=str)
    enrol_t, rest_t = verify.split_enrolment(args.target.glob("*.wav"), args.enroll_utts)
    enrol_s, rest_s = verify.split_enrolment(args.source.glob("*.wav"), args.enroll_utts)
    if not converted or not enrol_t or not enrol_s:
        print("ivector: needs *.wav files in the converted, the target and the source directory", file=sys.stderr)
        return 1
    models = np.stack([Backend.speaker(ex.embed(*verify._read(fs))) for fs in (enrol_t, enrol_s)])

    def rows(files, own):
        """per-file cosine rows and the decision for column `own` (0 target, 1 source)"""
        if not files:
            return [], verify.decide([], [])
        cos = cosine_scores(ex.embed(*verify._read(files)), models)
        d = verify.decide(cos[:, own], cos[:, 1 - own])
        return [dict(utterance=ev.utterance_id(f), file=str(f), cos_target=_num(a), cos_source=_num(b), accepted=flag)
                for f, (a, b), flag in zip(files, cos, d["flags"])], d

    conv, dc = rows(converted, 0)
    for r in conv:
        if r["accepted"] is None:
            print(f"utterance {r['utterance']} cos: nan (no voiced frames)")
        else:
            print(f"utterance {r['utterance']} cos: target {r['cos_target']} source {r['cos_source']}")
    mt = verify.finite_mean([r["cos_target"] for r in conv if r["accepted"] is not None])
    ms = verify.finite_mean([r["cos_source"] for r in conv if r["accepted"] is not None])
    print(f"target accepted: {dc['hits']}/{dc['scored']}")
    print(f"mean cos: target {mt} source {ms} over {dc['scored']} of {len(conv)} files")
    nat_t, dt = rows(rest_t, 0)
    nat_s, ds = rows(rest_s, 1)
    nat_hits, nat_scored = dt["hits"] + ds["hits"], dt["scored"] + ds["scored"]
    print(f"natural speech identified: {nat_hits}/{nat_scored}")
    result = dict(converted_dir=str(args.converted_dir), target=str(args.target), source=str(args.source),
                  ubm=str(args.ubm), ivector=str(args.ivector), components=ubm.K, rank=ex.rank,
                  enroll_utts=args.enroll_utts,
                  enrolled=dict(target=[str(f) for f in enrol_t], source=[str(f) for f in enrol_s]),
                  files=conv, accepted=dc["hits"], scored=dc["scored"], mean_cos_target=_num(mt), mean_cos_source=_num(ms),
                  no_voiced=[conv[i]["file"] for i in dc["unvoiced"]],
                  natural=dict(identified=nat_hits, scored=nat_scored, target=nat_t, source=nat_s,
                               no_voiced=[nat_t[i]["file"] for i in dt["unvoiced"]] +
                                         [nat_s[i]["file"] for i in ds["unvoiced"]]))
    (args.json or args.converted_dir.joinpath("ivector.json")).write_text(json.dumps(result, indent=1) + "\n")
    return 0


def _eer(args) -> int:
    if not args.wav16_root.is_dir():
        print(f"ivector: {args.wav16_root} is not a directory", file=sys.stderr)
        return 2
    ubm = DiagGMM.load(args.ubm)
    ex = Extractor.load(args.ivector, ubm)
    if ex.backend is None:
        print(f"ivector: {args.ivector} holds no backend", file=sys.stderr)
        return 1
    corpus = verify.corpus_files(args.wav16_root, args.max_utts_per_speaker)
    split = {sp: verify.split_enrolment(fs, args.enroll_utts) for sp, fs in corpus.items()}
    names = [sp for sp in split if split[sp][0]]
    trials = [(sp, f) for sp in names for f in split[sp][1]]
    if len(names) < 2 or not trials:
        print("ivector: needs two speakers or more, and files beyond the enrolment ones", file=sys.stderr)
        return 1
    v = verify.Verifier(ubm)
    models = []
    for sp in names:
        wavs, srs = verify._read(split[sp][0])
        models.append(Backend.speaker(ex.embed(wavs, srs)))
        v.enroll({sp: wavs}, {sp: srs})
    wavs, srs = verify._read([f for _, f in trials])
    cos, llr = cosine_scores(ex.embed(wavs, srs), np.stack(models)), v.llr(wavs, srs)
    own = np.array([[sp == name for name in names] for sp, _ in trials])
    fin = np.isfinite(cos).all(axis=1) & np.isfinite(llr).all(axis=1)
    no_voiced = [str(f) for (_, f), ok in zip(trials, fin) if not ok]
    if not (own & fin[:, None]).any() or not (~own & fin[:, None]).any():
        print("ivector: no trial with voiced frames", file=sys.stderr)
        return 1
    res = {}
    for key, sc in (("cosine", cos), ("llr", llr)):
        tar, non = sc[own & fin[:, None]], sc[~own & fin[:, None]]
        rate, thr = eer(tar, non)
        res[key] = dict(eer_percent=100.0 * rate, threshold=thr, target_trials=int(tar.size), nontarget_trials=int(non.size))
        print(f"eer {key}: {100.0 * rate} % ({tar.size} target, {non.size} non-target trials)")
    for f in no_voiced:
        print(f"no voiced frames: {f}")
    if args.json is not None:
        res.update(wav16_root=str(args.wav16_root), ubm=str(args.ubm), ivector=str(args.ivector), speakers=names,
                   enroll_utts=args.enroll_utts, no_voiced=no_voiced)
        args.json.write_text(json.dumps(res, indent=1) + "\n")
    return 0


def main(argv=None) -> int:
    args = _parse(sys.argv[1:] if argv is None else argv)
    return {"train": _train, "score": _score, "eer": _eer}[args.cmd](args)


if __name__ == "__main__":
    sys.exit(main())
