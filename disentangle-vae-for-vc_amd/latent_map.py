"""Latent map on the GPU: a 2-D neighbour embedding of the posterior means of a block (style, content or
both) and the leave-one-out 1-nearest-neighbour speaker agreement of the block, in the latent space and in the map.

    python -m dvae_amd.latent_map <corpus> --log_dir <run> [--block style|content|joint|all] [--level chunk|utterance]
        [--perplexity 30] [--iters 750] [--max_utts N] [--max-chunks M] [--seed S] [--init pca|random] [--use-ema]
        [--json PATH] [--no-svg]

The embedding is an exact t-SNE (van der Maaten & Hinton 2008) with scikit-learn's optimiser and defaults: per point a
precision beta_i at which p_{j|i} ~ exp(-beta_i d_ij) has the perplexity asked for (dvae_tsne_affinities), joint
probabilities p_ij = (p_{j|i} + p_{i|j}) / 2N, and gradient descent with momentum and gains on the KL divergence to
q_ij ~ 1 / (1 + |y_i - y_j|^2), early exaggeration first.  No N x N table exists: every iteration is one launch that
recomputes the distances and sums the forces of every row (dvae_tsne_forces) and one that adds the normalisation and moves
the points (dvae_tsne_update), with no host synchronisation; the KL of every `kl_every`-th iteration lands in a device
array that is downloaded once.

1-NN speaker agreement: the share of points whose nearest neighbour (dvae_tsne_nn) has the point's speaker, where chunks of
the point's own utterance are not admissible, so session and channel do not count; beside it chance = sum_g p_g^2.  A
non-parametric companion of `probe`: no classifier, no epochs, no split.  Rows with a non-finite value are taken out
first, counted and listed.  The picture is a self-contained SVG written here (no matplotlib); the same run gives the same
bytes.  GPU only.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path
from xml.sax.saxutils import escape

import numpy as np
import torch

from . import _lib
from .latents import MAX_D, encode_posteriors, list_chunks, subset
from .probe import N_MEL, checkpoint_files

MAX_STEPS = 64                # evaluations of the perplexity search
ENTROPY_TOL = 1e-5            # scikit-learn's; a constant of the kernel
EXAGGERATION = 12.0
MIN_LR = 50.0
KL_EVERY = 50
INIT_STD = 1e-4
PALETTE = ("#1f77b4", "#ff7f0e", "#2ca02c", "#d62728", "#9467bd", "#8c564b", "#e377c2", "#7f7f7f", "#bcbd22", "#17becf",
           "#393b79", "#637939", "#8c6d31", "#843c39", "#7b4173", "#3182bd", "#e6550d", "#31a354", "#756bb1", "#636363")
BLOCKS = ("style", "content", "joint")


def pca_init(x, seed: int = 0) -> np.ndarray:
    """the first two principal components of x [N, D] from the host float64 D x D covariance, scaled so that the first has
    a standard deviation of 1e-4; a component's sign makes its largest entry positive"""
    x = np.asarray(x, np.float64)
    xc = x - x.mean(0)
    N, D = x.shape
    if D < 2:
        y = np.concatenate([xc, np.random.default_rng(seed).standard_normal((N, 1))], axis=1)
    else:
        _, vec = np.linalg.eigh(xc.T @ xc / max(N - 1, 1))
        v = vec[:, ::-1][:, :2]
        v = v * np.where(v[np.abs(v).argmax(0), np.arange(2)] < 0, -1.0, 1.0)
        y = xc @ v
    sd = y[:, 0].std()
    return y / (sd if sd > 0 else 1.0) * INIT_STD


def nn_agreement(arg, speakers):
    """(the share of the rows with a neighbour whose neighbour has their speaker, the number of rows without one)"""
    arg, speakers = np.asarray(arg), np.asarray(speakers)
    has = arg >= 0
    if not has.any():
        return float("nan"), int((~has).sum())
    return float(np.mean(speakers[arg[has]] == speakers[has])), int((~has).sum())


def chance(speakers) -> float:
    _, n = np.unique(np.asarray(speakers), return_counts=True)
    p = n / n.sum()
    return float((p * p).sum())


def kl_of_rows(rows) -> float:
    """sum p ln p - sum p ln w + ln Z sum p from the eight sums of every row, float64 in row order"""
    r = np.asarray(rows, np.float64)
    acc = lambda v: float(np.add.accumulate(v)[-1])
    return acc(r[:, 5]) - acc(r[:, 6]) + math.log(acc(r[:, 4])) * acc(r[:, 7])


# ------------------------------------------------------------------------------------------------------------ the GPU
class LatentMap:
    """The four launches behind the map and the map itself.  Every tensor is fp32, contiguous, on `device`."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("LatentMap runs on the HIP path only (no CPU fallback)")

    def _f32(self, x):
        return torch.as_tensor(x).to(device=self.device, dtype=torch.float32).contiguous()

    def _x(self, x, what):
        x = self._f32(x)
        if x.dim() != 2 or not 1 <= x.shape[1] <= MAX_D or x.shape[0] < 1:
            raise ValueError(f"LatentMap.{what}: x [N, D] with 1 <= D <= {MAX_D}, got {tuple(x.shape)}")
        return x

    def nearest(self, x, group=None):
        """x [N, D], group [N] int or None -> (d2min [N] fp32, arg [N] int32): the nearest admissible neighbour
        (dvae_tsne_nn); +inf and -1 for a row without one"""
        x = self._x(x, "nearest")
        N, D = x.shape
        g = None
        if group is not None:
            g = torch.as_tensor(np.ascontiguousarray(group, dtype=np.int32)).to(self.device)
            if g.shape != (N,):
                raise ValueError(f"LatentMap.nearest: one group per row, got {tuple(g.shape)} for {N} rows")
        d2min = torch.empty(N, device=self.device, dtype=torch.float32)
        arg = torch.empty(N, device=self.device, dtype=torch.int32)
        _lib.check(_lib.lib().dvae_tsne_nn(x.data_ptr(), D, N, D, _lib.ptr(g), 0, N, d2min.data_ptr(), arg.data_ptr(),
                                           _lib.stream()), "dvae_tsne_nn")
        return d2min, arg

    def affinities(self, x, perplexity: float, max_steps: int = MAX_STEPS) -> dict:
        """x [N, D] -> {beta, d2min, lnz, entropy [N] fp32, steps [N] int32 (-1: not converged)} (dvae_tsne_nn without
        groups, then dvae_tsne_affinities)"""
        x = self._x(x, "affinities")
        N, D = x.shape
        if N - 1 < 3 * perplexity:
            raise ValueError(f"LatentMap.affinities: perplexity {perplexity} needs more than {3 * perplexity} neighbours, "
                             f"{N} points have {N - 1}")
        d2min, _ = self.nearest(x)
        beta, lnz, ent = (torch.empty(N, device=self.device, dtype=torch.float32) for _ in range(3))
        steps = torch.empty(N, device=self.device, dtype=torch.int32)
        _lib.check(_lib.lib().dvae_tsne_affinities(x.data_ptr(), D, N, D, d2min.data_ptr(), float(perplexity),
                                                   int(max_steps), 0, N, beta.data_ptr(), lnz.data_ptr(), ent.data_ptr(),
                                                   steps.data_ptr(), _lib.stream()), "dvae_tsne_affinities")
        return dict(beta=beta, d2min=d2min, lnz=lnz, entropy=ent, steps=steps)

    def forces(self, x, aff: dict, y, want_kl: bool = True) -> torch.Tensor:
        """the eight sums of every row at y [N, 2] -> rows [N, 8] (dvae_tsne_forces)"""
        N, D = x.shape
        rows = torch.empty((N, 8), device=self.device, dtype=torch.float32)
        _lib.check(_lib.lib().dvae_tsne_forces(x.data_ptr(), D, N, D, aff["beta"].data_ptr(), aff["d2min"].data_ptr(),
                                               aff["lnz"].data_ptr(), y.data_ptr(), int(bool(want_kl)), 0, N,
                                               rows.data_ptr(), _lib.stream()), "dvae_tsne_forces")
        return rows

    def embed(self, x, aff: dict, y0, iters: int, exaggeration_iters: int, exaggeration: float, lr: float,
              kl_every: int = KL_EVERY) -> dict:
        """gradient descent from y0 [N, 2]: `exaggeration_iters` iterations with the attraction times `exaggeration` and
        momentum 0.5, the rest with momentum 0.8 -> {y [N, 2] (device), kl (of the final y), kl_trace [(iteration, the KL
        before its update)]}.  Two launches an iteration, no host synchronisation before the end."""
        x = self._x(x, "embed")
        N, D = x.shape
        y = self._f32(y0).clone()
        if y.shape != (N, 2):
            raise ValueError(f"LatentMap.embed: y0 [N, 2], got {tuple(y.shape)}")
        if iters < 0 or kl_every < 1 or not lr > 0 or not exaggeration > 0:
            raise ValueError("LatentMap.embed: iters >= 0, kl_every >= 1, lr > 0, exaggeration > 0")
        upd, gains = torch.zeros_like(y), torch.ones_like(y)
        rows = torch.empty((N, 8), device=self.device, dtype=torch.float32)
        at = [it for it in range(iters) if it % kl_every == 0]
        kl = torch.zeros(max(len(at), 1), device=self.device, dtype=torch.float64)
        h, s = _lib.lib(), _lib.stream()
        ptrs = [aff[k].data_ptr() for k in ("beta", "d2min", "lnz")]
        for it in range(iters):
            early, want = it < exaggeration_iters, it % kl_every == 0
            _lib.check(h.dvae_tsne_forces(x.data_ptr(), D, N, D, *ptrs, y.data_ptr(), int(want), 0, N, rows.data_ptr(), s),
                       "dvae_tsne_forces")
            _lib.check(h.dvae_tsne_update(rows.data_ptr(), N, y.data_ptr(), upd.data_ptr(), gains.data_ptr(), float(lr),
                                          0.5 if early else 0.8, float(exaggeration) if early else 1.0,
                                          kl.data_ptr() + 8 * (it // kl_every) if want else None, s), "dvae_tsne_update")
        last = self.forces(x, aff, y, want_kl=True)
        torch.cuda.synchronize()
        trace = [(int(it), float(v)) for it, v in zip(at, kl.cpu().numpy())]
        return dict(y=y, kl=kl_of_rows(last.cpu().numpy()), kl_trace=trace)

    def map(self, x, speakers, groups, perplexity: float = 30.0, iters: int = 750, exaggeration_iters: int = 250,
            exaggeration: float = EXAGGERATION, lr=None, seed: int = 0, init: str = "pca", kl_every: int = KL_EVERY) -> dict:
        """x [N, D] (device or host), speakers [N], groups [N] (the utterance of a chunk) -> the map and its scores (a dict of
        plain Python values and numpy arrays; "_aff" holds the downloaded beta, d2min, lnz, entropy and steps and "_x" the
        kept rows)."""
        x = self._x(x, "map")
        speakers, groups = np.asarray(speakers).reshape(-1), np.asarray(groups).reshape(-1)
        N0 = x.shape[0]
        if len(speakers) != N0 or len(groups) != N0:
            raise ValueError("LatentMap.map: one speaker and one group per row")
        if init not in ("pca", "random"):
            raise ValueError(f"LatentMap.map: init {init!r}: pca or random")
        finite = torch.isfinite(x).all(dim=1)
        keep = finite.cpu().numpy()
        bad = np.flatnonzero(~keep)
        if len(bad):
            x, speakers, groups = x[finite].contiguous(), speakers[keep], groups[keep]
        N = int(x.shape[0])
        if N - 1 < 3 * perplexity:
            raise ValueError(f"LatentMap.map: perplexity {perplexity} needs more than {3 * perplexity} neighbours, "
                             f"{N} points have {N - 1}")
        aff = self.affinities(x, perplexity)
        xh = x.cpu().numpy()
        y0 = pca_init(xh, seed) if init == "pca" else np.random.default_rng(seed).standard_normal((N, 2)) * INIT_STD
        lr = max(N / exaggeration / 4.0, MIN_LR) if lr is None else float(lr)
        emb = self.embed(x, aff, y0.astype(np.float32), iters, exaggeration_iters, exaggeration, lr, kl_every)
        grp = np.unique(groups, return_inverse=True)[1].astype(np.int32)
        _, a_lat = self.nearest(x, grp)
        _, a_map = self.nearest(emb["y"], grp)
        torch.cuda.synchronize()
        affh = {k: v.cpu().numpy() for k, v in aff.items()}
        lat, none_lat = nn_agreement(a_lat.cpu().numpy(), speakers)
        mp, none_map = nn_agreement(a_map.cpu().numpy(), speakers)
        unconv = np.flatnonzero(affh["steps"] < 0)
        return dict(n_points=N, perplexity=float(perplexity), iters=int(iters), exaggeration_iters=int(exaggeration_iters),
                    exaggeration=float(exaggeration), lr=lr, seed=int(seed), init=init, y=emb["y"].cpu().numpy(),
                    kl=emb["kl"], kl_trace=emb["kl_trace"], unconverged=int(len(unconv)),
                    unconverged_rows=[int(i) for i in unconv],
                    nn_agreement=dict(latent=lat, map=mp, chance=chance(speakers)),
                    rows_without_neighbour=dict(latent=none_lat, map=none_map),
                    non_finite_rows=[int(i) for i in bad], kept=np.flatnonzero(keep), _aff=affh, _x=xh)


# ------------------------------------------------------------------------------------------------------------ the SVG
def svg_scatter(y, speakers, names, title: str = "", size: int = 640, margin: int = 24, legend: int = 150) -> str:
    """one circle per point on a `size` x `size` panel, a fixed palette indexed by speaker, a legend of the speaker names;
    coordinates with two decimals: the same input gives the same bytes"""
    y = np.asarray(y, np.float64)
    speakers = np.asarray(speakers)
    lo, hi = (y.min(0), y.max(0)) if len(y) else (np.zeros(2), np.ones(2))
    span = float(max((hi - lo).max(), 1e-30))
    mid = (lo + hi) / 2.0
    scale = (size - 2 * margin) / span
    out = [f'<svg xmlns="http://www.w3.org/2000/svg" width="{size + legend}" height="{size}" '
           f'viewBox="0 0 {size + legend} {size}">',
           f'<rect width="{size + legend}" height="{size}" fill="#ffffff"/>']
    if title:
        out.append(f'<text x="{margin}" y="16" font-family="sans-serif" font-size="12">{escape(title)}</text>')
    for (a, b), s in zip(y, speakers):
        px, py = size / 2.0 + (a - mid[0]) * scale, size / 2.0 - (b - mid[1]) * scale
        out.append(f'<circle cx="{px:.2f}" cy="{py:.2f}" r="2.5" fill="{PALETTE[int(s) % len(PALETTE)]}" fill-opacity="0.7"/>')
    for k, name in enumerate(names):
        ty = margin + 16 * k
        if ty > size - margin:
            break
        out.append(f'<rect x="{size + 8}" y="{ty - 9}" width="10" height="10" fill="{PALETTE[k % len(PALETTE)]}"/>')
        out.append(f'<text x="{size + 24}" y="{ty}" font-family="sans-serif" font-size="11">{escape(str(name))}</text>')
    out.append("</svg>")
    return "\n".join(out) + "\n"


# ---------------------------------------------------------------------------------------------------------------- CLI
def map_line(block: str, r: dict) -> str:
    a = r["nn_agreement"]
    x0 = r["kl_trace"][0][1] if r["kl_trace"] else r["kl"]
    return (f"latent map {block}: {r['n_points']} points, perplexity {r['perplexity']}, kl {r['kl']} (from {x0}), "
            f"1-nn speaker agreement: latent {a['latent']}, map {a['map']} (chance {a['chance']}), "
            f"unconverged rows {r['unconverged']}")


def utterance_means(mu, utt) -> tuple:
    """the float64 mean of every utterance's chunk means, in chunk order -> (means [U, D] fp32, the utterances' ids)"""
    ids, inv = np.unique(utt, return_inverse=True)
    mu = np.asarray(mu, np.float64)
    sums, cnt = np.zeros((len(ids), mu.shape[1])), np.zeros(len(ids))
    np.add.at(sums, inv, mu)
    np.add.at(cnt, inv, 1.0)
    return (sums / cnt[:, None]).astype(np.float32), ids


class _Parser(argparse.ArgumentParser):
    def error(self, message):
        raise ValueError(message)


def _parse(argv):
    p = _Parser(prog="python -m dvae_amd.latent_map",
                description="2-D t-SNE map of the latents of a trained run and their 1-NN speaker agreement, on the GPU.")
    p.add_argument("corpus", type=Path, help="<corpus>/<speaker>/*.npy mels [80, L] (what --dataset_fp of train.py reads)")
    p.add_argument("--log_dir", type=Path, required=True, help="the run: config.json and checkpoints/ of train.py")
    p.add_argument("--block", choices=BLOCKS + ("all",), default="all")
    p.add_argument("--level", choices=("chunk", "utterance"), default="chunk")
    p.add_argument("--perplexity", type=float, default=30.0)
    p.add_argument("--iters", type=int, default=750)
    p.add_argument("--max_utts", type=int, default=None, help="use the first N sorted utterances of every speaker")
    p.add_argument("--max-chunks", type=int, default=16384, help="a seeded subset of the chunks, in speaker order")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--init", choices=("pca", "random"), default="pca")
    p.add_argument("--use-ema", action="store_true", default=False,
                   help="encode with the averaged weights (<name>_<epoch>.ema.pth of a --ema-decay run)")
    p.add_argument("--json", type=Path, default=None, help="where to write the results (default <log_dir>/latent_map.json)")
    p.add_argument("--no-svg", action="store_true", default=False)
    return p.parse_args(argv)


def main(argv=None) -> int:
    err = lambda msg: print(f"latent_map: {msg}", file=sys.stderr)
    try:
        args = _parse(sys.argv[1:] if argv is None else argv)
    except ValueError as e:
        err(str(e))
        return 2
    if args.max_chunks < 1 or (args.max_utts is not None and args.max_utts < 1):
        err("--max-chunks and --max_utts are at least 1")
        return 2
    if not args.perplexity >= 1.0 or args.iters < 1:
        err("--perplexity is at least 1 and --iters at least 1")
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
    spans = dict(style=(0, S), content=(S, latent), joint=(0, latent))
    blocks = [b for b in (BLOCKS if args.block == "all" else (args.block,)) if spans[b][1] > spans[b][0]]
    if not blocks:
        err(f"--block {args.block}: the block has no dimensions (latent_size {latent}, speaker_size {S})")
        return 2
    try:
        chunks = list_chunks(args.corpus, T, args.max_utts)
    except ValueError as e:
        err(str(e))
        return 2
    if not torch.cuda.is_available():
        err("no GPU: the map runs on the HIP path only")
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
    mu, _ = encode_posteriors(vsc, chunks, index)
    torch.cuda.synchronize()
    vsc._check_device_errors()
    utt, spk = chunks.utt[index], chunks.speaker[index]
    if args.level == "utterance":
        pts, ids = utterance_means(mu.cpu().numpy(), utt)
        first = np.array([np.flatnonzero(utt == u)[0] for u in ids])
        spk, grp = spk[first], np.arange(len(ids))
    else:
        pts, grp = mu, utt
    lm = LatentMap(device)
    names, lines, results = chunks.speakers, [], {}
    for b in blocks:
        lo, hi = spans[b]
        try:
            r = lm.map(pts[:, lo:hi], spk, grp, perplexity=args.perplexity, iters=args.iters,
                       exaggeration_iters=min(250, args.iters // 3), seed=args.seed, init=args.init)
        except ValueError as e:
            err(str(e))
            return 2
        r.pop("_aff")
        r.pop("_x")
        y, kept = r.pop("y"), r.pop("kept")
        np.save(args.log_dir.joinpath(f"latent_map_{b}.npy"), y)
        if not args.no_svg:
            args.log_dir.joinpath(f"latent_map_{b}.svg").write_text(svg_scatter(y, spk[kept], names, title=map_line(b, r)))
        line = map_line(b, r)
        print(line)
        lines.append(line)
        results[b] = r
    result = dict(corpus=str(args.corpus), log_dir=str(args.log_dir), checkpoint_epoch=int(next_epoch) - 1, n_frames=T,
                  use_ema=bool(args.use_ema), level=args.level, max_utts=args.max_utts, max_chunks=args.max_chunks,
                  n_corpus_chunks=len(chunks), speakers=names, skipped=list(chunks.skipped), style_dims=S,
                  blocks=results, lines=lines)
    out_path = args.json or args.log_dir.joinpath("latent_map.json")
    out_path.write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
