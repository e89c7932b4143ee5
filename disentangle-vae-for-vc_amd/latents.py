"""Latent report on the GPU: has the posterior collapsed, how much information do the latents carry and
is it factorised, how much do the style and the content block share, and how many nats of speaker identity sit in each?

    python -m dvae_amd.latents <corpus> --log_dir <run> [--max_utts N] [--max-chunks M] [--seed S] [--use-ema] [--json PATH]

The eval-mode encoder gives the posterior N(mu_j, exp lv_j) of every full chunk of the corpus, D = latent_dim wide: the
first S = speaker_size columns are the style block, the rest the content block.  One sample per chunk,
z_i = mu_i + exp(lv_i / 2) eps_i (eps: float32 of np.random.default_rng(seed).standard_normal), and the N x N x D table of
t_ijd = log q(z_id | x_j) with its log-sum-exps over j (dvae_latent_lse, csrc/latents.hip) give, as means over i
(Chen et al. 2018, the decomposition of the mean KL, over the whole corpus instead of a minibatch):

    mi      mean(own - (L_joint - ln N))                 index-code mutual information I(z; chunk), at most ln N
    tc      mean((L_joint - ln N) - sum_d (L_d - ln N))  total correlation of the aggregate posterior
    dwkl    mean(sum_d (L_d - ln N) - prior)             dimension-wise KL to the prior
    shared  mean(L_joint - L_style - L_content + ln N)   what the two blocks share under the aggregate posterior
    speaker information of a block   mean((L_block over the chunks of i's own speaker - ln n_g) - (L_block - ln N)),
            beside H = -sum p_g ln p_g of the chunk counts; speakers with fewer than 8 chunks are listed and left out

mi + tc + dwkl = mean(own - prior) is an identity of the definitions and is asserted.  The same three are given for each block
alone.  The estimator counts the sample's own component among the N: mi cannot exceed ln N (printed beside it), and
quantities that are zero for independent variables come out slightly positive (a few hundredths of a nat at a thousand
chunks).  There is no leave-one-out correction.  Host float64 beside them, per dimension: the analytic
kl_d = mean (mu^2 + e^lv - lv - 1) / 2, the variance of mu_d over the chunks, the mean posterior variance, and the active
units of Burda et al. (var_i(mu_id) > 0.01).  Chunks with a non-finite mu, lv or table entry are taken out of rows and
columns before the launch, counted and listed.  GPU only; the same corpus and seed give the same bits.
"""
from __future__ import annotations

import argparse
import glob
import json
import math
import os
import sys
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import _lib
from .probe import Chunks, HELD_OUT_EVERY, N_MEL, checkpoint_files

MAX_D = 64                    # DVAE_LATENT_MAX_D
ACTIVE_VAR = 0.01
MIN_SPEAKER_CHUNKS = 8
LOG_2PI = math.log(2.0 * math.pi)


# ---------------------------------------------------------------------------------------------------------- host side
def list_chunks(corpus, n_frames: int, max_utts: Optional[int] = None) -> Chunks:
    """probe.list_chunks' listing (the same layout, order and probe.Chunks) without its demands on the split: the report
    trains nothing, so a speaker needs neither five utterances nor a held-out one."""
    corpus = str(corpus)
    speakers = sorted(d for d in os.listdir(corpus) if os.path.isdir(os.path.join(corpus, d)))
    if not speakers:
        raise ValueError(f"{corpus}: no speaker directories")
    utterances, skipped, utt, start, spk, held = [], [], [], [], [], []
    for s, name in enumerate(speakers):
        files = sorted(glob.glob(os.path.join(corpus, name, "*.npy")))
        for i, fp in enumerate(files[:int(max_utts)] if max_utts is not None else files):
            shape = np.load(fp, mmap_mode="r").shape
            if len(shape) != 2 or shape[0] != N_MEL:
                raise ValueError(f"{fp}: expected a [{N_MEL}, L] mel, got {tuple(shape)}")
            n = int(shape[1]) // n_frames
            if n < 1:
                skipped.append(fp)
                continue
            ho = i % HELD_OUT_EVERY == HELD_OUT_EVERY - 1
            utterances.append(dict(path=fp, speaker=s, position=i, length=int(shape[1]), n_chunks=n, held_out=ho))
            utt += [len(utterances) - 1] * n
            start += [k * n_frames for k in range(n)]
            spk += [s] * n
            held += [ho] * n
    if not utt:
        raise ValueError(f"{corpus}: no utterance of at least {n_frames} frames")
    return Chunks(n_frames=int(n_frames), speakers=speakers, utterances=utterances, utt=np.asarray(utt, dtype=np.int64),
                  start=np.asarray(start, dtype=np.int64), speaker=np.asarray(spk, dtype=np.int32),
                  held_out=np.asarray(held, dtype=bool), skipped=skipped)


def subset(chunks: Chunks, max_chunks: Optional[int], seed: int) -> np.ndarray:
    """indices of at most max_chunks chunks drawn by default_rng(seed) without replacement, ascending: the speaker order
    stays"""
    n = len(chunks)
    if max_chunks is None or n <= max_chunks:
        return np.arange(n, dtype=np.int64)
    return np.sort(np.random.default_rng(seed).choice(n, size=int(max_chunks), replace=False)).astype(np.int64)


def encode_posteriors(vsc, chunks: Chunks, index=None, batch: int = 256):
    """eval-mode `encode_heads` over the chunks `index` (default: all) -> (mu [n, D], lv [n, D]) on the device, the style
    head's S columns first"""
    m = vsc.model
    S, Cn = m.speaker_size, m.latent_dim - m.speaker_size
    index = np.arange(len(chunks)) if index is None else np.asarray(index)
    n, T, dev = len(index), chunks.n_frames, vsc.device
    mu = torch.empty((n, S + Cn), device=dev, dtype=torch.float32)
    lv = torch.empty((n, S + Cn), device=dev, dtype=torch.float32)
    was_training = m.training
    m.eval()
    try:
        with torch.no_grad():
            cur, mel = -1, None
            for at in range(0, n, batch):
                ids = index[at:at + batch]
                buf = np.empty((len(ids), N_MEL, T), dtype=np.float32)
                for k, c in enumerate(ids):
                    u = int(chunks.utt[c])
                    if u != cur:
                        cur, mel = u, np.load(chunks.utterances[u]["path"])
                    buf[k] = mel[:, chunks.start[c]:chunks.start[c] + T]
                st, ct = m.encode_heads(torch.from_numpy(buf).to(dev))          # [b, 2S], [b, 2Cn]: mu | logvar
                mu[at:at + len(ids), :S], lv[at:at + len(ids), :S] = st[:, :S], st[:, S:]
                mu[at:at + len(ids), S:], lv[at:at + len(ids), S:] = ct[:, :Cn], ct[:, Cn:]
    finally:
        m.train(was_training)
    return mu, lv


def _mean(v) -> float:
    """float64 mean, the terms added in chunk order"""
    v = np.asarray(v, np.float64)
    return float(np.add.accumulate(v)[-1] / len(v)) if len(v) else float("nan")


def speaker_runs(speakers) -> list:
    """sorted labels [n] -> [(label, first row, count)] per run"""
    speakers = np.asarray(speakers)
    first = np.concatenate([[0], np.flatnonzero(np.diff(speakers)) + 1]).astype(np.int64)
    count = np.diff(np.concatenate([first, [len(speakers)]]))
    return [(int(speakers[f]), int(f), int(c)) for f, c in zip(first, count)]


# ------------------------------------------------------------------------------------------------------------ the GPU
class LatentReport:
    """The two launches behind the report and the report itself.  Every tensor is fp32, contiguous, on `device`."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("LatentReport runs on the HIP path only (no CPU fallback)")

    def _f32(self, x):
        return torch.as_tensor(x).to(device=self.device, dtype=torch.float32).contiguous()

    def tables(self, mu, lv, eps) -> dict:
        """mu, lv, eps [N, D] -> {z, mu, a, h} [N, D] (dvae_latent_tables)"""
        mu, lv, eps = self._f32(mu), self._f32(lv), self._f32(eps)
        if mu.dim() != 2 or mu.shape != lv.shape or mu.shape != eps.shape:
            raise ValueError(f"LatentReport.tables: mu, lv, eps [N, D], got {tuple(mu.shape)}, {tuple(lv.shape)}, {tuple(eps.shape)}")
        N, D = mu.shape
        if not 1 <= D <= MAX_D:
            raise ValueError(f"LatentReport.tables: D = {D}; the kernels take 1 .. {MAX_D}")
        z, a, h = torch.empty_like(mu), torch.empty_like(mu), torch.empty_like(mu)
        _lib.check(_lib.lib().dvae_latent_tables(mu.data_ptr(), lv.data_ptr(), eps.data_ptr(), z.data_ptr(), a.data_ptr(),
                                                 h.data_ptr(), N, D, D, _lib.stream()), "dvae_latent_tables")
        return dict(z=z, mu=mu, a=a, h=h)

    def lse(self, tables: dict, jobs, S: int = 0) -> torch.Tensor:
        """jobs [njobs][5] {row0, nrows, col0, ncols, out0} -> out [max(out0 + nrows), D + 3] (dvae_latent_lse): per row
        the D per-dimension LSEs, then style (d < S), content, joint.  Rows no job writes hold NaN."""
        z, mu, a, h = (tables[k] for k in ("z", "mu", "a", "h"))
        N, D = z.shape
        jobs = np.ascontiguousarray(np.asarray(jobs, dtype=np.int64).reshape(-1, 5))
        if not len(jobs):
            raise ValueError("LatentReport.lse: no jobs")
        if (jobs < 0).any() or (jobs[:, 3] < 1).any() or (jobs[:, 0] + jobs[:, 1] > N).any() or (jobs[:, 2] + jobs[:, 3] > N).any():
            raise ValueError("LatentReport.lse: a job's rows or columns lie outside the tables, or it has no columns")
        if not 0 <= S <= D:
            raise ValueError(f"LatentReport.lse: S = {S} with D = {D}")
        rows = int((jobs[:, 4] + jobs[:, 1]).max())
        out = torch.full((rows, D + 3), float("nan"), device=self.device, dtype=torch.float32)
        jd = torch.from_numpy(jobs).to(self.device)
        _lib.check(_lib.lib().dvae_latent_lse(z.data_ptr(), mu.data_ptr(), a.data_ptr(), h.data_ptr(), D, D, int(S),
                                              jd.data_ptr(), jobs.ctypes.data, len(jobs), out.data_ptr(), D + 3,
                                              _lib.stream()), "dvae_latent_lse")
        return out

    def report(self, mu, lv, speakers, S: int, seed: int = 0, eps=None) -> dict:
        """mu, lv [N, D] (device or host), speakers [N] sorted labels, S the style block's width -> the report (a dict of
        plain Python values; "_tables" and "_lse" hold the downloaded fp32 tables and LSE tables of the kept chunks).
        eps: the draws to use in place of default_rng(seed)'s."""
        mu, lv = self._f32(mu), self._f32(lv)
        N0, D = mu.shape
        speakers = np.asarray(speakers).reshape(-1)
        if len(speakers) != N0 or (np.diff(speakers) < 0).any():
            raise ValueError("LatentReport.report: one speaker label per chunk, sorted")
        if not 0 <= S <= D:
            raise ValueError(f"LatentReport.report: S = {S} with D = {D}")
        if eps is None:
            eps = np.random.default_rng(seed).standard_normal((N0, D)).astype(np.float32)
        t = self.tables(mu, lv, np.ascontiguousarray(eps, dtype=np.float32))
        finite = torch.isfinite(torch.stack([t["z"], t["mu"], t["a"], t["h"], lv])).all(dim=0).all(dim=1)
        bad = np.flatnonzero(~finite.cpu().numpy())
        if len(bad):
            t = {k: v[finite].contiguous() for k, v in t.items()}
            lv, speakers = lv[finite].contiguous(), speakers[finite.cpu().numpy()]
        N = int(t["z"].shape[0])
        if N < 1:
            raise ValueError("LatentReport.report: no chunk with finite posteriors")
        runs = speaker_runs(speakers)
        jobs = [[0, N, 0, N, 0]] + [[r, n, r, n, N + r] for _, r, n in runs]
        out = self.lse(t, jobs, S)
        torch.cuda.synchronize()
        L = out.cpu().numpy().astype(np.float64)
        tabs = {k: v.cpu().numpy() for k, v in t.items()}
        res = quantities(tabs, lv.cpu().numpy(), L[:N], L[N:], speakers, S)
        res.update(seed=int(seed), n_chunks=N, non_finite_chunks=[int(i) for i in bad], _tables=tabs, _lse=L)
        return res


def quantities(tabs: dict, lv, L_all, L_own, speakers, S: int) -> dict:
    """host float64 from the fp32 tables, the global job's LSE table and the speakers' jobs' -> the report's figures"""
    z, mu, a, h = (np.asarray(tabs[k], np.float64) for k in ("z", "mu", "a", "h"))
    lv = np.asarray(lv, np.float64)
    N, D = z.shape
    lnN = math.log(N)
    own_d = a - h * (z - mu) ** 2
    prior_d = -0.5 * LOG_2PI - 0.5 * z * z
    Ld = L_all[:, :D] - lnN
    kl_d = 0.5 * (mu * mu + np.exp(lv) - lv - 1.0)
    var_mu = mu.var(axis=0)
    res = dict(ln_n=lnN, blocks={})
    for name, lo, hi, col in (("style", 0, S, D), ("content", S, D, D + 1), ("joint", 0, D, D + 2)):
        own, prior, marg = own_d[:, lo:hi].sum(1), prior_d[:, lo:hi].sum(1), Ld[:, lo:hi].sum(1)
        Lb = L_all[:, col] - lnN
        b = dict(dims=hi - lo, kl=_mean(kl_d[:, lo:hi].sum(1)), active_units=int((var_mu[lo:hi] > ACTIVE_VAR).sum()),
                 mi=_mean(own - Lb), tc=_mean(Lb - marg), dwkl=_mean(marg - prior), kl_sample=_mean(own - prior))
        gap = abs(b["mi"] + b["tc"] + b["dwkl"] - b["kl_sample"])
        assert gap <= 1e-9 * (1.0 + abs(b["kl_sample"]) + abs(b["mi"]) + abs(b["tc"]) + abs(b["dwkl"])), (name, gap)
        res["blocks"][name] = b
    res["shared"] = _mean(L_all[:, D + 2] - L_all[:, D] - L_all[:, D + 1] + lnN)
    runs = speaker_runs(speakers)
    keep, ln_ng = np.zeros(N, bool), np.zeros(N, np.float64)
    for _, r, n in runs:
        keep[r:r + n] = n >= MIN_SPEAKER_CHUNKS
        ln_ng[r:r + n] = math.log(n)
    p = np.array([n for _, _, n in runs], np.float64) / N
    res["speaker_entropy"] = float(-(p * np.log(p)).sum())
    res["speaker_chunks"] = {int(g): int(n) for g, _, n in runs}
    res["small_speakers"] = [int(g) for g, _, n in runs if n < MIN_SPEAKER_CHUNKS]
    res["speaker_info"] = {name: _mean(((L_own[:, col] - ln_ng) - (L_all[:, col] - lnN))[keep])
                           for name, col in (("style", D), ("content", D + 1))}
    res["dimensions"] = [dict(d=d, block="style" if d < S else "content", kl=_mean(kl_d[:, d]), var_mu=float(var_mu[d]),
                              mean_var=_mean(np.exp(lv[:, d])), active=bool(var_mu[d] > ACTIVE_VAR),
                              marginal_kl=_mean(Ld[:, d] - prior_d[:, d])) for d in range(D)]
    return res


# ------------------------------------------------------------------------------------------------------------------ CLI
def report_lines(res: dict) -> list:
    out = []
    for name in ("style", "content", "joint"):
        b = res["blocks"][name]
        out.append(f"latents {name}: kl {b['kl']} nats, active units {b['active_units']}/{b['dims']}, mi {b['mi']} "
                   f"(ln N = {res['ln_n']}), tc {b['tc']}, dwkl {b['dwkl']}")
    out.append(f"style/content shared information: {res['shared']} nats")
    si = res["speaker_info"]
    out.append(f"speaker information: style {si['style']}, content {si['content']} of H = {res['speaker_entropy']} nats")
    out.append("dimension block kl var_mu mean_var active marginal_kl")
    for r in res["dimensions"]:
        out.append(f"dimension {r['d']} {r['block']} {r['kl']} {r['var_mu']} {r['mean_var']} {int(r['active'])} {r['marginal_kl']}")
    return out


class _Parser(argparse.ArgumentParser):
    def error(self, message):
        raise ValueError(message)


def _parse(argv):
    p = _Parser(prog="python -m dvae_amd.latents",
                description="KL decomposition, collapse and speaker leakage of the latents of a trained run, on the GPU.")
    p.add_argument("corpus", type=Path, help="<corpus>/<speaker>/*.npy mels [80, L] (what --dataset_fp of train.py reads)")
    p.add_argument("--log_dir", type=Path, required=True, help="the run: config.json and checkpoints/ of train.py")
    p.add_argument("--max_utts", type=int, default=None, help="use the first N sorted utterances of every speaker")
    p.add_argument("--max-chunks", type=int, default=32768, help="a seeded subset of the chunks, in speaker order")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--use-ema", action="store_true", default=False,
                   help="encode with the averaged weights (<name>_<epoch>.ema.pth of a --ema-decay run)")
    p.add_argument("--json", type=Path, default=None, help="where to write the results (default <log_dir>/latents.json)")
    return p.parse_args(argv)


def main(argv=None) -> int:
    err = lambda msg: print(f"latents: {msg}", file=sys.stderr)
    try:
        args = _parse(sys.argv[1:] if argv is None else argv)
    except ValueError as e:
        err(str(e))
        return 2
    if args.max_chunks < 1 or (args.max_utts is not None and args.max_utts < 1):
        err("--max-chunks and --max_utts are at least 1")
        return 2
    cfg_path = args.log_dir.joinpath("config.json")
    if not cfg_path.is_file():
        err(f"{cfg_path} is missing: --log_dir must be the --log_dir of a python -m dvae_amd.train run")
        return 2
    if not args.corpus.is_dir():
        err(f"{args.corpus} is not a directory")
        return 2
    cfg = json.loads(cfg_path.read_text())
    ckpt_dir = args.log_dir.joinpath("checkpoints")
    if not checkpoint_files(ckpt_dir):
        err(f"no checkpoint under {ckpt_dir}: train the model first (python -m dvae_amd.train --train true "
            f"--log_dir {args.log_dir})")
        return 1
    T = int(cfg.get("samples_length", 64))
    latent, S = int(cfg.get("latent_size", 32)), int(cfg.get("speaker_size", 4))
    if not (1 <= latent <= MAX_D and 0 <= S <= latent):
        err(f"latent_size {latent}, speaker_size {S}: the kernels take up to {MAX_D} dimensions")
        return 2
    try:
        chunks = list_chunks(args.corpus, T, args.max_utts)
    except ValueError as e:
        err(str(e))
        return 2
    if not torch.cuda.is_available():
        err("no GPU: the report runs on the HIP path only")
        return 2
    from .model.disentangled_vae import ConvolutionalMulVAE
    device = torch.device("cuda", torch.cuda.current_device())
    vsc = ConvolutionalMulVAE(cfg.get("dataset", "VCTK"), T, N_MEL, latent, float(cfg.get("lr", 1e-3)),
                              float(cfg.get("alpha", 0.01)), int(cfg.get("log_interval", 500)),
                              bool(cfg.get("normalize", False)), speaker_size=S, device=device, latent_dim=latent,
                              beta=float(cfg.get("beta_cof", 0.1)), batch_size=int(cfg.get("batch_size", 2)),
                              mse_cof=float(cfg.get("mse_cof", 10)), kl_cof=float(cfg.get("kl_cof", 10)),
                              style_cof=float(cfg.get("style_cof", 0.1)))
    try:
        next_epoch = vsc.load_last_model(str(ckpt_dir), logging_func=lambda *_: None, use_ema=args.use_ema)
    except FileNotFoundError as e:
        err(f"--use-ema: {e}")
        return 1
    index = subset(chunks, args.max_chunks, args.seed)
    mu, lv = encode_posteriors(vsc, chunks, index)
    torch.cuda.synchronize()
    vsc._check_device_errors()
    res = LatentReport(device).report(mu, lv, chunks.speaker[index], S, seed=args.seed)
    res.pop("_tables")
    res.pop("_lse")
    names = chunks.speakers
    res["speaker_chunks"] = {names[g]: n for g, n in res["speaker_chunks"].items()}
    res["small_speakers"] = [names[g] for g in res["small_speakers"]]
    res["non_finite_chunks"] = [int(index[i]) for i in res["non_finite_chunks"]]
    lines = report_lines(res)
    for line in lines:
        print(line)
    if res["small_speakers"]:
        print(f"speakers with fewer than {MIN_SPEAKER_CHUNKS} chunks (left out of the speaker information): "
              + ", ".join(res["small_speakers"]))
    if res["non_finite_chunks"]:
        print(f"non-finite chunks left out: {len(res['non_finite_chunks'])}")
    result = dict(corpus=str(args.corpus), log_dir=str(args.log_dir), checkpoint_epoch=int(next_epoch) - 1, n_frames=T,
                  use_ema=bool(args.use_ema), max_utts=args.max_utts, max_chunks=args.max_chunks,
                  n_corpus_chunks=len(chunks), speakers=names, skipped=list(chunks.skipped), style_dims=S, **res,
                  lines=lines)
    out_path = args.json or args.log_dir.joinpath("latents.json")
    out_path.write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
