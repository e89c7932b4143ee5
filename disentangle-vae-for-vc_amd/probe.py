"""Speaker-identity probe of the style and content latents on the GPU: does the STYLE latent
carry the speaker while the CONTENT latent does not?

    python -m dvae_amd.probe <corpus> --log_dir <run> [--max_utts N] [--epochs E] [--seed S] [--json PATH]
                                      [--score DIR --speaker NAME] [--use-ema]

The reference's hook is a speaker classifier on latents, model/feature_selection.py:5-43 trained by
model/train_feature_selection.py:10-61 — written for an older model (`sparse_encoding`, 512-wide latents), with a softmax
in front of `cross_entropy` — and the per-speaker latent statistics of model/plot.py:23-44.  Restated here for the
disentangled VAE: the eval-mode encoder gives `style_mu` and `content_mu` of every full chunk of the corpus, and one small
classifier per latent (Linear -> ReLU -> Linear, ops.LinearFn; loss, gradient, arg-max and sums by dvae_softmax_ce,
csrc/probe.hip; optim.FlatAdam) is fitted to predict the speaker.  Its accuracy on HELD-OUT UTTERANCES is the figure:
near 1 for a style latent that identifies the speaker, near chance (1 / speakers) for a content latent that does not.

    chunks      every utterance [80, L] gives L // n_frames full chunks; no zero-padded tail; shorter utterances are skipped
    split       by utterance, never by chunk: position i in the speaker's sorted file list is held out when i % 5 == 4
    features    standardised by the training chunks' per-dimension mean and standard deviation (+ 1e-6)
    classifier  hidden 1024, Adam lr 1e-3, 30 epochs of minibatches of 4096 from one seeded permutation per epoch
    --score     converted .wav files (16 kHz) -> mel -> full chunks -> style_mu -> the style probe's mean log-probability
                over a file's chunks; the arg-max is the predicted speaker, reported against --speaker

The --score figure uses the model's OWN encoder: it says whether the model recognises its conversion as the target
speaker, not whether an independent listener or speaker-verification network would.  GPU only, no CPU
fallback; no plotting.
"""
from __future__ import annotations

import argparse
import glob
import json
import math
import os
import sys
from dataclasses import dataclass, field
from pathlib import Path
from typing import List, Optional

import numpy as np
import torch

HELD_OUT_EVERY = 5            # position i of a speaker's sorted utterances is held out when i % 5 == 4
MIN_UTTERANCES = 5            # usable utterances a speaker needs
N_MEL = 80


def pad_width(n: int) -> int:
    """Feature and class counts rounded up to the contraction kernels' 16-byte operand rows (4 floats).  K = 4 is taken
    as it is."""
    return (int(n) + 3) // 4 * 4


# --------------------------------------------------------------------------------------------------------- host side
@dataclass
class Chunks:
    """The chunk list of a corpus (list_chunks).  Per-chunk arrays are ordered by speaker, utterance, start frame."""
    n_frames: int
    speakers: List[str]
    utterances: List[dict]                # {path, speaker (index), position, length, n_chunks, held_out}
    utt: np.ndarray                       # [n] index into `utterances`
    start: np.ndarray                     # [n] first frame of the chunk
    speaker: np.ndarray                   # [n] int32 label
    held_out: np.ndarray                  # [n] bool
    skipped: List[str] = field(default_factory=list)      # utterances shorter than n_frames

    def __len__(self):
        return int(self.utt.shape[0])


def list_chunks(corpus, n_frames: int, max_utts: Optional[int] = None) -> Chunks:
    """`<corpus>/<speaker>/*.npy` with arrays [80, L] (the layout data.SpeechDatasetGVAE reads; speakers are the sorted
    sub-directories, a speaker's files are sorted and cut to `max_utts`) -> every full chunk of n_frames frames."""
    corpus = str(corpus)
    speakers = sorted(d for d in os.listdir(corpus) if os.path.isdir(os.path.join(corpus, d)))
    if not speakers:
        raise ValueError(f"{corpus}: no speaker directories")
    utterances, skipped = [], []
    utt, start, spk, held = [], [], [], []
    for s, name in enumerate(speakers):
        files = sorted(glob.glob(os.path.join(corpus, name, "*.npy")))
        if max_utts is not None:
            files = files[:int(max_utts)]
        usable = 0
        for i, fp in enumerate(files):
            shape = np.load(fp, mmap_mode="r").shape
            if len(shape) != 2 or shape[0] != N_MEL:
                raise ValueError(f"{fp}: expected a [{N_MEL}, L] mel, got {tuple(shape)}")
            n = int(shape[1]) // n_frames
            if n < 1:
                skipped.append(fp)
                continue
            usable += 1
            ho = i % HELD_OUT_EVERY == HELD_OUT_EVERY - 1
            utterances.append(dict(path=fp, speaker=s, position=i, length=int(shape[1]), n_chunks=n, held_out=ho))
            utt += [len(utterances) - 1] * n
            start += [k * n_frames for k in range(n)]
            spk += [s] * n
            held += [ho] * n
        if usable < MIN_UTTERANCES:
            raise ValueError(f"speaker {name}: {usable} utterances of at least {n_frames} frames; the probe needs "
                             f"{MIN_UTTERANCES} per speaker (a held-out utterance and training utterances)")
        sides = {u["held_out"] for u in utterances if u["speaker"] == s}
        if sides != {False, True}:
            raise ValueError(f"speaker {name}: no {'held-out' if True not in sides else 'training'} utterance is left "
                             f"after skipping those shorter than {n_frames} frames")
    return Chunks(n_frames=int(n_frames), speakers=speakers, utterances=utterances,
                  utt=np.asarray(utt, dtype=np.int64), start=np.asarray(start, dtype=np.int64),
                  speaker=np.asarray(spk, dtype=np.int32), held_out=np.asarray(held, dtype=bool), skipped=skipped)


def checkpoint_files(checkpoints_path) -> list:
    """the files load_last_model would choose from: `<name>_<tag>_<epoch>.pth`"""
    out = []
    for f in glob.glob(f"{checkpoints_path}/*.pth"):
        parts = Path(f).stem.split("_")
        if len(parts) == 3 and parts[2].isdigit():
            out.append(f)
    return sorted(out)


# ----------------------------------------------------------------------------------------------------------- encoder
def _encode(vsc, batches, n: int):
    """batches: iterable of host float32 arrays [b, 80, T] or device tensors -> (style_mu [n, S], content_mu [n, Cn])"""
    m = vsc.model
    S, Cn = m.speaker_size, m.latent_dim - m.speaker_size
    dev = vsc.device
    style = torch.empty((n, S), device=dev, dtype=torch.float32)
    content = torch.empty((n, Cn), device=dev, dtype=torch.float32)
    was_training = m.training
    m.eval()
    try:
        with torch.no_grad():
            at = 0
            for xb in batches:
                xb = torch.as_tensor(xb).to(device=dev, dtype=torch.float32).contiguous()
                st, ct = m.encode_heads(xb)          # [b, 2S], [b, 2Cn]: mu | logvar
                b = xb.shape[0]
                style[at:at + b].copy_(st[:, :S])
                content[at:at + b].copy_(ct[:, :Cn])
                at += b
            if at != n:
                raise RuntimeError(f"encoded {at} of {n} chunks")
    finally:
        m.train(was_training)
    return style, content


def encode_corpus(vsc, chunks: Chunks, batch: int = 256):
    """eval-mode `encode_heads` over every chunk, `batch` at a time -> (style_mu [n, S], content_mu [n, Cn]) on the device"""
    T = chunks.n_frames

    def batches():
        buf, fill, cur, mel = np.empty((batch, N_MEL, T), dtype=np.float32), 0, -1, None
        for u, s0 in zip(chunks.utt, chunks.start):
            if u != cur:
                cur, mel = u, np.load(chunks.utterances[u]["path"])
            buf[fill] = mel[:, s0:s0 + T]
            fill += 1
            if fill == batch:
                yield buf
                fill = 0
        if fill:
            yield buf[:fill]

    return _encode(vsc, batches(), len(chunks))


# -------------------------------------------------------------------------------------------------------- classifier
class SpeakerProbe:
    """Linear(dim_p, hidden) -> ReLU -> Linear(hidden, classes_p) through ops.LinearFn, trained with ops.SoftmaxCeFn and
    optim.FlatAdam (lr 1e-3).  dim_p / classes_p: dim / n_speakers padded to a multiple of 4 (pad_width); padding feature
    columns are zero, padding classes are masked by the kernel's `classes` argument, and the padding rows and columns of
    the parameters start at zero and stay there (their gradients are exactly zero).  Initialisation: nn.Linear's default
    (U(+-1/sqrt(fan_in)) for weight and bias, fan_in = dim / hidden) drawn from a CPU generator seeded with `seed`."""

    def __init__(self, dim: int, n_speakers: int, hidden: int = 1024, seed: int = 0, device="cuda", lr: float = 1e-3):
        from . import ops
        from .optim import FlatAdam
        if dim < 1 or n_speakers < 1 or hidden < 4 or hidden % 4:
            raise ValueError("SpeakerProbe: dim, n_speakers >= 1 and hidden a positive multiple of 4")
        if n_speakers > ops.CE_MAX_CLASSES:
            raise ValueError(f"SpeakerProbe: {n_speakers} speakers; the loss kernel takes up to {ops.CE_MAX_CLASSES}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("SpeakerProbe runs on the HIP path only (no CPU fallback)")
        self.dim, self.n_speakers, self.hidden, self.seed = int(dim), int(n_speakers), int(hidden), int(seed)
        self.dim_p, self.classes_p = pad_width(dim), pad_width(n_speakers)
        g = torch.Generator(device="cpu")
        g.manual_seed(self.seed)

        def draw(rows, cols, rows_p, cols_p, fan_in):
            b = 1.0 / math.sqrt(fan_in)
            w = torch.zeros(rows_p, cols_p)
            w[:rows, :cols] = torch.empty(rows, cols).uniform_(-b, b, generator=g)
            bias = torch.zeros(rows_p)
            bias[:rows] = torch.empty(rows).uniform_(-b, b, generator=g)
            return w, bias

        w1, b1 = draw(self.hidden, self.dim, self.hidden, self.dim_p, self.dim)
        w2, b2 = draw(self.n_speakers, self.hidden, self.classes_p, self.hidden, self.hidden)
        self.params = {k: torch.nn.Parameter(v.to(self.device)) for k, v in (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2))}
        self.optimizer = FlatAdam(list(self.params.items()), lr=lr)
        self.mean = torch.zeros(self.dim, device=self.device, dtype=torch.float32)
        self.std = torch.ones(self.dim, device=self.device, dtype=torch.float32)
        self.epoch_losses: List[float] = []

    # ---- features
    def standardise(self, x) -> torch.Tensor:
        """x [n, dim] -> (x - mean) / (std + 1e-6), zero-padded to [n, dim_p]"""
        x = torch.as_tensor(x).to(device=self.device, dtype=torch.float32)
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"SpeakerProbe: expected features [n, {self.dim}], got {tuple(x.shape)}")
        out = torch.zeros((x.shape[0], self.dim_p), device=self.device, dtype=torch.float32)
        out[:, :self.dim] = (x - self.mean) / (self.std + 1e-6)
        return out

    def _labels(self, y) -> np.ndarray:
        y = y.cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
        y = np.ascontiguousarray(y.reshape(-1), dtype=np.int32)
        if y.size and y.max() >= self.n_speakers:
            raise ValueError(f"SpeakerProbe: label {int(y.max())} with {self.n_speakers} speakers")
        return y

    def logits(self, xs) -> torch.Tensor:
        """standardised, padded features [n, dim_p] -> logits [n, classes_p] (columns >= n_speakers are padding)"""
        from .ops import ACT_NONE, ACT_RELU, LinearFn
        p = self.params
        h = LinearFn.apply(xs, p["w1"], p["b1"], ACT_RELU)
        return LinearFn.apply(h, p["w2"], p["b2"], ACT_NONE)

    def loss(self, xs, y_dev, count: int) -> torch.Tensor:
        """mean cross-entropy of the `count` rows with a label >= 0 (a device scalar with a gradient)"""
        from .ops import SoftmaxCeFn
        return SoftmaxCeFn.apply(self.logits(xs), y_dev, self.n_speakers, count)

    # ---- training
    def fit(self, x, y, epochs: int = 30, batch: int = 4096, logging_func=None):
        """x [n, dim] features (device tensor or array), y [n] speaker labels (host).  Returns the mean loss per epoch."""
        y = self._labels(y)
        x = torch.as_tensor(x).to(device=self.device, dtype=torch.float32)
        n = x.shape[0]
        if n < 1 or n != y.shape[0]:
            raise ValueError("SpeakerProbe.fit: one label per feature row, at least one row")
        x64 = x.double()
        self.mean = x64.mean(0).float()
        self.std = x64.std(0, unbiased=False).float()
        xs = self.standardise(x)
        y_dev = torch.from_numpy(y).to(self.device)
        self.epoch_losses = []
        opt = self.optimizer
        for epoch in range(int(epochs)):
            perm = np.random.RandomState(self.seed + epoch).permutation(n)
            perm_dev = torch.from_numpy(perm).to(self.device)
            tot = torch.zeros((), device=self.device, dtype=torch.float64)
            counted = 0
            for i in range(0, n, int(batch)):
                idx = perm_dev[i:i + batch]
                count = int((y[perm[i:i + batch]] >= 0).sum())
                if count < 1:
                    continue
                opt.zero_grad()
                loss = self.loss(xs.index_select(0, idx), y_dev.index_select(0, idx), count)
                loss.backward()
                opt.step()
                tot += loss.detach().double() * count
                counted += count
            mean_loss = float(tot.item()) / max(1, counted)      # one host synchronisation per epoch
            self.epoch_losses.append(mean_loss)
            if logging_func is not None:
                logging_func(f"probe epoch {epoch + 1}: mean loss {mean_loss:.6f}")
        return self.epoch_losses

    # ---- evaluation
    def _eval_batches(self, x, batch):
        xs = self.standardise(x)
        with torch.no_grad():
            for i in range(0, xs.shape[0], batch):
                yield i, self.logits(xs[i:i + batch])

    def evaluate(self, x, y, batch: int = 8192) -> dict:
        """-> {loss, accuracy, n} over the rows with a label >= 0"""
        from .ops import softmax_ce_eval
        y_dev = torch.from_numpy(self._labels(y)).to(self.device)
        tot = torch.zeros(3, device=self.device, dtype=torch.float64)
        for i, lg in self._eval_batches(x, batch):
            tot += softmax_ce_eval(lg, y_dev[i:i + batch], self.n_speakers).double()
        s, n, k = tot.tolist()
        return dict(loss=s / n if n else float("nan"), accuracy=k / n if n else float("nan"), n=int(n))

    def predict(self, x, batch: int = 8192) -> torch.Tensor:
        """arg-max speaker of every row, int32 [n] on the device"""
        from .ops import softmax_ce
        out = torch.empty(torch.as_tensor(x).shape[0], device=self.device, dtype=torch.int32)
        none = torch.full((min(batch, max(1, out.shape[0])),), -1, device=self.device, dtype=torch.int32)
        for i, lg in self._eval_batches(x, batch):
            out[i:i + lg.shape[0]] = softmax_ce(lg, none[:lg.shape[0]], self.n_speakers, reduce=False)[1]
        return out

    def log_prob(self, x, batch: int = 8192) -> torch.Tensor:
        """log-softmax over the speakers, [n, n_speakers] on the device: the kernel's log-sum-exp (the row loss against
        class 0 plus that class's logit) taken off the logits"""
        from .ops import softmax_ce
        n = torch.as_tensor(x).shape[0]
        out = torch.empty((n, self.n_speakers), device=self.device, dtype=torch.float32)
        zero = torch.zeros(min(batch, max(1, n)), device=self.device, dtype=torch.int32)
        for i, lg in self._eval_batches(x, batch):
            nll0 = softmax_ce(lg, zero[:lg.shape[0]], self.n_speakers, reduce=False)[0]
            out[i:i + lg.shape[0]] = lg[:, :self.n_speakers] - (nll0 + lg[:, 0])[:, None]
        return out


# ------------------------------------------------------------------------------------------------------------------ CLI
def probe_latent(name: str, z, chunks: Chunks, epochs: int, seed: int, logging_func=None) -> tuple:
    """fit one probe on the training chunks of latent z [n, dim] -> (probe, result dict)"""
    S = len(chunks.speakers)
    tr, ho = np.flatnonzero(~chunks.held_out), np.flatnonzero(chunks.held_out)
    sel = lambda idx: z.index_select(0, torch.from_numpy(idx).to(z.device))
    z_tr, z_ho = sel(tr), sel(ho)
    y_tr, y_ho = chunks.speaker[tr], chunks.speaker[ho]
    probe = SpeakerProbe(z.shape[1], S, seed=seed, device=z.device)
    probe.fit(z_tr, y_tr, epochs=epochs, logging_func=logging_func)
    e_tr, e_ho = probe.evaluate(z_tr, y_tr), probe.evaluate(z_ho, y_ho)
    hit = probe.predict(z_ho).cpu().numpy() == y_ho
    per = {spk: float(hit[y_ho == s].mean()) for s, spk in enumerate(chunks.speakers)}
    n_utt = sum(1 for u in chunks.utterances if u["held_out"])
    res = dict(latent=name, dim=int(z.shape[1]), held_out_accuracy=e_ho["accuracy"], train_accuracy=e_tr["accuracy"],
               held_out_loss=e_ho["loss"], train_loss=e_tr["loss"], chance=1.0 / S, n_held_out_chunks=e_ho["n"],
               n_train_chunks=e_tr["n"], n_held_out_utterances=n_utt, n_speakers=S, per_speaker_held_out_accuracy=per,
               epoch_losses=list(probe.epoch_losses))
    return probe, res


def probe_line(res: dict) -> str:
    return (f"probe {res['latent']}: held-out accuracy {res['held_out_accuracy']:.4f} (train {res['train_accuracy']:.4f}, "
            f"chance {res['chance']:.4f}, {res['n_held_out_chunks']} held-out chunks of {res['n_held_out_utterances']} "
            f"utterances, {res['n_speakers']} speakers)")


def style_statistics(style_mu, chunks: Chunks) -> dict:
    """per speaker the mean and standard deviation of every style dimension over the speaker's chunks (float64, host):
    the data behind the reference's latent plots, model/plot.py:23-44"""
    z = style_mu.cpu().numpy().astype(np.float64)
    out = {}
    for s, spk in enumerate(chunks.speakers):
        zs = z[chunks.speaker == s]
        out[spk] = dict(n_chunks=int(zs.shape[0]), mean=zs.mean(0).tolist(), std=zs.std(0).tolist())
    return out


def score_directory(vsc, probe: SpeakerProbe, chunks: Chunks, wav_dir, speaker: str) -> dict:
    """--score: every .wav of wav_dir (16 kHz) -> mel -> full chunks -> style_mu -> mean log-probability per file"""
    from .frontend import MelFrontend
    from .preprocess import read_wav
    T = chunks.n_frames
    files = sorted(Path(wav_dir).glob("*.wav"))
    if not files:
        raise ValueError(f"{wav_dir}: no .wav files")
    wavs = []
    for f in files:
        w, sr = read_wav(f)
        if int(sr) != 16000:
            raise ValueError(f"{f}: {sr} Hz; --score reads 16 kHz files (python -m dvae_amd.preprocess resamples)")
        wavs.append(w)
    mels = MelFrontend(device=vsc.device).melspectrogram_batch(wavs)          # [80, M_i] on the device
    counts = [int(m.shape[1]) // T for m in mels]
    rows = [m[:, k * T:(k + 1) * T] for m, c in zip(mels, counts) for k in range(c)]
    result = dict(dir=str(wav_dir), speaker=speaker, files=[], skipped=[], correct=0, n=0)
    lp = None
    if rows:
        style, _ = _encode(vsc, [torch.stack(rows[i:i + 256]) for i in range(0, len(rows), 256)], len(rows))
        lp = probe.log_prob(style).cpu().numpy().astype(np.float64)
    at = 0
    for f, c in zip(files, counts):
        if c < 1:
            result["skipped"].append(f.name)
            print(f"file {f.name}: skipped (shorter than one chunk of {T} frames)")
            continue
        pred = chunks.speakers[int(np.argmax(lp[at:at + c].mean(0)))]
        at += c
        result["files"].append(dict(file=f.name, predicted=pred, n_chunks=c))
        result["n"] += 1
        result["correct"] += int(pred == speaker)
        print(f"file {f.name}: {pred}")
    print(f"target speaker accuracy: {result['correct']}/{result['n']}")
    return result


def _parse(argv):
    p = argparse.ArgumentParser(prog="python -m dvae_amd.probe",
                                description="Speaker-identity probe of the style and content latents of a trained run, "
                                            "on the GPU.")
    p.add_argument("corpus", type=Path, help="<corpus>/<speaker>/*.npy mels [80, L] (what --dataset_fp of train.py reads)")
    p.add_argument("--log_dir", type=Path, required=True, help="the run: config.json and checkpoints/ of train.py")
    p.add_argument("--max_utts", type=int, default=None, help="use the first N sorted utterances of every speaker")
    p.add_argument("--epochs", type=int, default=30)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--json", type=Path, default=None, help="where to write the results (default <log_dir>/probe.json)")
    p.add_argument("--score", type=Path, default=None, help="directory of converted 16 kHz .wav files to classify")
    p.add_argument("--speaker", type=str, default=None, help="--score: the target speaker (a directory name of the corpus)")
    p.add_argument("--use-ema", action="store_true", default=False,
                   help="encode with the averaged weights (<name>_<epoch>.ema.pth of a --ema-decay run)")
    return p.parse_args(argv)


def main(argv=None) -> int:
    args = _parse(sys.argv[1:] if argv is None else argv)
    err = lambda msg: print(f"probe: {msg}", file=sys.stderr)
    cfg_path = args.log_dir.joinpath("config.json")
    if not cfg_path.is_file():
        err(f"{cfg_path} is missing: --log_dir must be the --log_dir of a python -m dvae_amd.train run")
        return 2
    cfg = json.loads(cfg_path.read_text())
    ckpt_dir = args.log_dir.joinpath("checkpoints")
    if not checkpoint_files(ckpt_dir):
        err(f"no checkpoint under {ckpt_dir}: train the model first (python -m dvae_amd.train --train true "
            f"--log_dir {args.log_dir})")
        return 1
    if not args.corpus.is_dir():
        err(f"{args.corpus} is not a directory")
        return 2
    if (args.score is None) != (args.speaker is None):
        err("--score DIR and --speaker NAME go together")
        return 2
    if args.score is not None and not args.score.is_dir():
        err(f"{args.score} is not a directory")
        return 2
    T = int(cfg.get("samples_length", 64))
    try:
        chunks = list_chunks(args.corpus, T, args.max_utts)
    except ValueError as e:
        err(str(e))
        return 2
    if args.speaker is not None and args.speaker not in chunks.speakers:
        err(f"--speaker {args.speaker} is not a speaker of {args.corpus}")
        return 2

    from .model.disentangled_vae import ConvolutionalMulVAE
    if not torch.cuda.is_available():
        err("no GPU: the probe runs on the HIP path only")
        return 2
    device = torch.device("cuda", torch.cuda.current_device())
    latent = int(cfg.get("latent_size", 32))
    vsc = ConvolutionalMulVAE(cfg.get("dataset", "VCTK"), T, N_MEL, latent, float(cfg.get("lr", 1e-3)),
                              float(cfg.get("alpha", 0.01)), int(cfg.get("log_interval", 500)),
                              bool(cfg.get("normalize", False)), speaker_size=int(cfg.get("speaker_size", 4)), device=device,
                              latent_dim=latent, beta=float(cfg.get("beta_cof", 0.1)),
                              batch_size=int(cfg.get("batch_size", 2)), mse_cof=float(cfg.get("mse_cof", 10)),
                              kl_cof=float(cfg.get("kl_cof", 10)), style_cof=float(cfg.get("style_cof", 0.1)))
    try:
        next_epoch = vsc.load_last_model(str(ckpt_dir), logging_func=lambda *_: None, use_ema=args.use_ema)
    except FileNotFoundError as e:
        err(f"--use-ema: {e}")
        return 1
    style_mu, content_mu = encode_corpus(vsc, chunks)
    torch.cuda.synchronize()
    vsc._check_device_errors()
    n_ho_utt = sum(1 for u in chunks.utterances if u["held_out"])
    result = dict(corpus=str(args.corpus), log_dir=str(args.log_dir), checkpoint_epoch=int(next_epoch) - 1, n_frames=T,
                  use_ema=bool(args.use_ema), seed=args.seed, epochs=args.epochs, max_utts=args.max_utts, speakers=chunks.speakers,
                  chance=1.0 / len(chunks.speakers), n_train_chunks=int((~chunks.held_out).sum()),
                  n_held_out_chunks=int(chunks.held_out.sum()), n_train_utterances=len(chunks.utterances) - n_ho_utt,
                  n_held_out_utterances=n_ho_utt, skipped=list(chunks.skipped), probes={})
    style_probe = None
    for name, z in (("style", style_mu), ("content", content_mu)):
        probe, res = probe_latent(name, z, chunks, args.epochs, args.seed)
        style_probe = probe if name == "style" else style_probe
        result["probes"][name] = res
        print(probe_line(res))
    result["style_stats"] = style_statistics(style_mu, chunks)
    if args.score is not None:
        try:
            result["score"] = score_directory(vsc, style_probe, chunks, args.score, args.speaker)
        except ValueError as e:
            err(str(e))
            return 2
    out_path = args.json or args.log_dir.joinpath("probe.json")
    out_path.write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
