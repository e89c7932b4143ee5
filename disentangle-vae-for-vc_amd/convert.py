"""Whole-utterance voice conversion: overlapped windows, cross-faded on the device, wav to wav.

The model sees fixed windows of T frames.  `convert_mel` (the reference's voice_conversion_mel) cuts an utterance into
L // T + 1 disjoint chunks and joins the decoded chunks with torch.cat: a seam every T frames, n T frames out instead of L,
the style of one target utterance.  Here an utterance of L frames is covered by windows `hop` frames apart, the last one moved
back to end at frame L (`window_plan`); the decoded windows are cross-faded with a sin^2 window and normalised by the
overlap-added window itself (dvae_windows_overlap_add), so the output has exactly L frames and no frame depends on one
window's border alone; the style is the float64 mean of style_mu over every window of every utterance of a speaker
(`StyleBank`), and `style_mix` blends it with the source's own mean.

    python -m dvae_amd.convert --log_dir RUN --source a.wav dir/ --target b.wav c.wav -o OUT

reads the model of a `python -m dvae_amd.train` run, turns the wavs into mels on the corpus's own path (resample to 16 kHz,
normalise the volume, mel front-end: preprocess._run_batch), converts every source to the mean style of all targets and
writes OUT/convert_<stem>.wav (Griffin-Lim, 16 kHz mono PCM-16, the resampled source's sample count) and convert_<stem>.npy.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path
from typing import Sequence

import numpy as np
import torch

from ._lib import check, lib, ptr, stream
from .packed import pad4, upload

N_MEL = 80


# ------------------------------------------------------------------------------------------------------------ host plan
def window_plan(L: int, T: int, hop: int) -> np.ndarray:
    """Starts (int64, strictly increasing) of the windows of T frames that cover an utterance of L frames: every `hop` frames
    while a whole window still fits before the last one, which ends at frame L — no window of an utterance with L >= T holds
    padding.  L < T: one window at 0, zero-padded on the right (as dvae_gather_crop pads a short training crop)."""
    L, T, hop = int(L), int(T), int(hop)
    if L < 1 or T < 1 or not 1 <= hop <= T:
        raise ValueError(f"window_plan: L={L}, T={T}, hop={hop}: L >= 1 and 1 <= hop <= T")
    return np.asarray(list(range(0, L - T, hop)) + [max(0, L - T)], dtype=np.int64)


def crossfade_window(T: int) -> np.ndarray:
    """w[j] = sin^2(pi (j + 1/2) / T), float64 [T]: strictly positive (the normalisation never divides by zero), symmetric,
    and w[j] + w[j + T/2] = 1 (at hop = T/2 the windows sum to one by themselves)."""
    return np.sin(np.pi * (np.arange(int(T), dtype=np.float64) + 0.5) / int(T)) ** 2


def flat_plan(lengths: Sequence[int], T: int, hop: int, batch: int = 1) -> dict:
    """One flattened window list for utterances of `lengths` frames packed as [C, ld]:
      utt [nutt, 4] int32 {col0, L, win0, nwin}: utterance u owns columns [col0, col0 + L), col0 a multiple of 4, and windows
                                                 win0 ... win0 + nwin - 1;
      win [nwin_padded, 2] int32 {utt, frame0}:  the windows of utterance 0, then of 1, ...; the list is filled up to a
                                                 multiple of `batch` with padding windows {-1, 0};
      ld: the packed width (>= 4), nwin: the windows that are not padding."""
    if not len(lengths) or int(batch) < 1:
        raise ValueError("flat_plan: at least one utterance and batch >= 1")
    utt = np.zeros((len(lengths), 4), dtype=np.int32)
    wins, col = [], 0
    for u, L in enumerate(lengths):
        starts = window_plan(L, T, hop)
        utt[u] = (col, int(L), len(wins), len(starts))
        wins += [(u, int(s)) for s in starts]
        col += pad4(int(L))
    nwin = len(wins)
    wins += [(-1, 0)] * (-nwin % int(batch))
    return dict(utt=utt, win=np.asarray(wins, dtype=np.int32).reshape(-1, 2), ld=max(4, col), nwin=nwin,
                T=int(T), hop=int(hop))


# --------------------------------------------------------------------------------------------------------- the launches
def _i32(t, n, what):
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n):
        raise ValueError(f"{what}: a contiguous int32 GPU tensor of {n} elements")


def _f32(t, what):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f"{what}: a contiguous fp32 GPU tensor")


def mel_to_windows(mels, utt_table, win_table, T: int):
    """dvae_mel_to_windows: mels [C, ld] packed, the two device tables of `flat_plan` -> [nwin, C, T]"""
    _f32(mels, "mel_to_windows: mels")
    C, ld = mels.shape
    nwin = win_table.shape[0]
    _i32(utt_table, utt_table.shape[0] * 4, "mel_to_windows: utt_table")
    _i32(win_table, nwin * 2, "mel_to_windows: win_table")
    out = torch.empty((nwin, C, int(T)), device=mels.device, dtype=torch.float32)
    check(lib().dvae_mel_to_windows(ptr(mels), ld, ptr(utt_table), ptr(win_table), ptr(out), nwin, C, int(T), stream()),
          "dvae_mel_to_windows")
    return out


def window_latents(content, sums, counts, g_src, g_trg, mix: float, S: int, counts_host=None):
    """dvae_window_latents: content [nwin, 2 Cn], sums [G, K] float64, counts [G] int64, g_src / g_trg [nwin] int32 ->
    z [nwin, S + Cn].  counts_host (the same counts on the host): a group in use that is empty is DVAE_EINVAL before the
    launch."""
    _f32(content, "window_latents: content")
    nwin, Cn = content.shape[0], content.shape[1] // 2
    _i32(g_src, nwin, "window_latents: g_src")
    _i32(g_trg, nwin, "window_latents: g_trg")
    G, K = sums.shape
    if not (sums.is_cuda and sums.dtype == torch.float64 and sums.is_contiguous() and counts.is_cuda
            and counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() == G):
        raise ValueError("window_latents: sums [G, K] float64 and counts [G] int64, contiguous on the GPU")
    if counts_host is not None:
        used = np.unique(np.concatenate([g_src.cpu().numpy(), g_trg.cpu().numpy()]))
        used = used[used >= 0]
        if used.size and (used.max() >= G or (np.asarray(counts_host)[used] < 1).any()):
            check(-1, "dvae_window_latents (a style group in use is empty or out of range)")
    z = torch.empty((nwin, int(S) + Cn), device=content.device, dtype=torch.float32)
    check(lib().dvae_window_latents(ptr(content), ptr(sums), ptr(counts), ptr(g_src), ptr(g_trg), float(mix), ptr(z), nwin,
                                    int(S), Cn, K, stream()), "dvae_window_latents")
    return z


def windows_overlap_add(y, utt_table, win_table, window, ld: int, clamp=None, out=None):
    """dvae_windows_overlap_add: y [nwin, C, T], `window` [T] fp32 -> out [C, ld] (columns that no utterance owns keep what
    `out` held: torch.empty by default); clamp: None or (lo, hi)"""
    _f32(y, "windows_overlap_add: y")
    _f32(window, "windows_overlap_add: window")
    nwin, C, T = y.shape
    nutt = utt_table.shape[0]
    _i32(utt_table, nutt * 4, "windows_overlap_add: utt_table")
    _i32(win_table, nwin * 2, "windows_overlap_add: win_table")
    if window.numel() != T:
        raise ValueError("windows_overlap_add: one window weight per frame of a window")
    if out is None:
        out = torch.empty((C, int(ld)), device=y.device, dtype=torch.float32)
    lo, hi = (0.0, 0.0) if clamp is None else clamp
    check(lib().dvae_windows_overlap_add(ptr(y), ptr(utt_table), ptr(win_table), ptr(window), ptr(out), int(ld), nutt, C, T,
                                         float(lo), float(hi), int(clamp is not None), stream()), "dvae_windows_overlap_add")
    return out


# ------------------------------------------------------------------------------------------------------------ the bank
class StyleBank:
    """Per-speaker style: the float64 sums of the style heads (mu | logvar, K = 2 S columns) over every window of every
    utterance of a group, and the window counts.  Data only: `save` writes an .npz that `load` reads without pickle."""

    def __init__(self, names, sums, counts, T, hop, S, checkpoint=""):
        self.names = [str(n) for n in names]
        self.sums = np.ascontiguousarray(sums, dtype=np.float64).reshape(len(self.names), -1)
        self.counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(len(self.names))
        self.T, self.hop, self.S, self.checkpoint = int(T), int(hop), int(S), str(checkpoint)

    def index(self, name) -> int:
        if name not in self.names:
            raise KeyError(f"StyleBank: no style group {name!r} (it holds {self.names})")
        return self.names.index(name)

    def mean(self, name) -> np.ndarray:
        """style_mu of a group, float64 [S]"""
        g = self.index(name)
        return self.sums[g, :self.S] / self.counts[g]

    def save(self, path) -> str:
        path = str(path)
        path = path if path.endswith(".npz") else path + ".npz"
        np.savez(path, names=np.asarray(self.names, dtype=np.str_), sums=self.sums, counts=self.counts,
                 T=np.int64(self.T), hop=np.int64(self.hop), S=np.int64(self.S), checkpoint=np.str_(self.checkpoint))
        return path

    @classmethod
    def load(cls, path) -> "StyleBank":
        with np.load(str(path), allow_pickle=False) as f:
            return cls([str(n) for n in f["names"]], f["sums"], f["counts"], int(f["T"]), int(f["hop"]), int(f["S"]),
                       str(f["checkpoint"]))


# ---------------------------------------------------------------------------------------------------------- the engine
class Converter:
    """Whole-utterance conversion on a trainer's model.

    Every forward runs in model.eval() at ONE shape: window i of the flattened list (`flat_plan`) is row i % batch of forward
    i // batch, and the last forward is filled with padding windows whose rows are dropped — the rule of `validate`, for the
    same reason: the contraction kernels choose tiles and splits by shape and the resident recurrence adds in an order that
    turns with the row, so a window's last bits depend on its forward's shape and on its row.  What this gives: the same
    list of utterances, the same `batch` and the same `hop` produce the same bits from run to run; another list (an
    utterance more, another order) may move an utterance's last bits, because its windows land in other rows."""

    def __init__(self, trainer, hop=None, batch: int = 32, checkpoint: str = ""):
        m = trainer.model
        self.trainer, self.model = trainer, m
        self.T, self.S, self.Cn = int(m.n_frames), int(m.speaker_size), int(m.latent_dim - m.speaker_size)
        self.hop = self.T // 2 if hop is None else int(hop)
        self.batch = int(batch)
        if not 1 <= self.hop <= self.T or self.batch < 1:
            raise ValueError(f"Converter: hop={self.hop} must lie in [1, {self.T}] and batch={self.batch} be >= 1")
        self.device = torch.device(trainer.device)
        if self.device.type != "cuda":
            raise RuntimeError("Converter runs on the HIP path only (no CPU fallback)")
        self.checkpoint = str(checkpoint)
        self.window = upload(crossfade_window(self.T), self.device)

    # ---- pieces (the engine test composes the same launches by hand)
    def _mel(self, mel):
        t = torch.as_tensor(mel).to(self.device, torch.float32)
        if t.dim() != 2 or t.shape[0] != N_MEL or t.shape[1] < 1:
            raise ValueError(f"Converter: a mel must be [{N_MEL}, L >= 1], not {tuple(t.shape)}")
        return t

    def pack(self, mels: Sequence):
        """list of [80, L] -> (plan with the tables on the device as plan['utt_d'], plan['win_d'], packed [80, ld])"""
        ms = [self._mel(m) for m in mels]
        plan = flat_plan([int(m.shape[1]) for m in ms], self.T, self.hop, self.batch)
        packed = torch.zeros((N_MEL, plan["ld"]), device=self.device, dtype=torch.float32)
        for m, (col0, L, _, _) in zip(ms, plan["utt"]):
            packed[:, col0:col0 + L] = m
        plan["utt_d"] = upload(plan["utt"], self.device, np.int32)
        plan["win_d"] = upload(plan["win"], self.device, np.int32)
        return plan, packed

    def encode(self, windows):
        """[n batch, 80, T] -> (style [n batch, 2 S], content [n batch, 2 Cn]), one encode_heads per `batch` rows"""
        n, B = windows.shape[0], self.batch
        style = torch.empty((n, 2 * self.S), device=self.device, dtype=torch.float32)
        content = torch.empty((n, 2 * self.Cn), device=self.device, dtype=torch.float32)
        for a in range(0, n, B):
            s, c = self.model.encode_heads(windows[a:a + B])
            style[a:a + B].copy_(s)
            content[a:a + B].copy_(c)
        return style, content

    def decode(self, z):
        """z [n batch, S + Cn] -> (decoded [n batch, 80, T], decoded + post-net), one decode and one post-net per `batch` rows"""
        n, B = z.shape[0], self.batch
        dec = torch.empty((n, N_MEL, self.T), device=self.device, dtype=torch.float32)
        post = torch.empty_like(dec)
        for a in range(0, n, B):
            d = self.model.decode(z[a:a + B])
            dec[a:a + B].copy_(d)
            post[a:a + B].copy_(self.model.postnet.forward_plus_input(d))
        return dec, post

    def group_sums(self, style, group, G: int):
        """float64 sums [G, 2 S] and counts [G] of the style rows per group (dvae_group_sum_f64; a group < 0 counts nowhere)"""
        from . import ops
        sums = torch.zeros((G + 1, style.shape[1]), dtype=torch.float64, device=self.device)
        counts = torch.zeros(2 * (G + 1), dtype=torch.int64, device=self.device)
        ops.group_sum(style, group, sums, counts[:G + 1], counts[G + 1:])
        return sums[:G].contiguous(), counts[:G].contiguous()

    def _eval(self):
        m = self.model

        class _Ctx:
            def __enter__(s):
                s.was, s.ng = m.training, torch.no_grad()
                m.eval()
                s.ng.__enter__()

            def __exit__(s, *exc):
                s.ng.__exit__(*exc)
                m.train(s.was)
        return _Ctx()

    # ---- the style bank
    def style_bank(self, mels_by_name: dict) -> StyleBank:
        """{name: [mel [80, L], ...]} -> StyleBank: every window of every utterance of a group through encode_heads, the
        style heads summed per group in float64."""
        names = list(mels_by_name)
        mels, owner = [], []
        for g, name in enumerate(names):
            group = mels_by_name[name]
            group = [group] if (torch.is_tensor(group) or isinstance(group, np.ndarray)) and group.ndim == 2 else list(group)
            if not group:
                raise ValueError(f"style_bank: group {name!r} is empty")
            mels += group
            owner += [g] * len(group)
        if not mels:
            raise ValueError("style_bank: no style group")
        with self._eval():
            plan, packed = self.pack(mels)
            style, _ = self.encode(mel_to_windows(packed, plan["utt_d"], plan["win_d"], self.T))
            u = plan["win"][:, 0]
            group = np.where(u >= 0, np.asarray(owner, dtype=np.int32)[np.maximum(u, 0)], -1).astype(np.int32)
            sums, counts = self.group_sums(style, upload(group, self.device, np.int32), len(names))
            sums, counts = sums.cpu().numpy(), counts.cpu().numpy()
        self.trainer._check_device_errors()
        empty = [n for n, c in zip(names, counts) if c < 1]
        if empty:
            raise ValueError(f"style_bank: no finite style window in {empty}")
        return StyleBank(names, sums, counts, self.T, self.hop, self.S, self.checkpoint)

    def check_bank(self, bank: StyleBank):
        if bank.T != self.T or bank.S != self.S or bank.sums.shape[1] != 2 * self.S:
            raise ValueError(f"StyleBank of a model with T={bank.T}, S={bank.S} (checkpoint {bank.checkpoint!r}); this model "
                             f"has T={self.T}, S={self.S}")

    # ---- conversion
    # ---- over-smoothing (modspec.py)
    def smoothing_stats(self, targets_by_name: dict, bank: StyleBank, modspec=None) -> tuple:
        """{name: [mel [80, L], ...]} of the bank's groups -> (natural, generated), two ModSpecStats: the natural statistics of
        the target mels, and those of the same files converted to their own group's style, self.convert(mels, name,
        bank)["converted"] — the model's smoothing response on that speaker.  modspec: a ModSpec (default: D = 64)."""
        from .modspec import ModSpec
        ms = ModSpec(self.device) if modspec is None else modspec
        one = lambda g: [g] if (torch.is_tensor(g) or isinstance(g, np.ndarray)) and g.ndim == 2 else list(g)
        groups = {name: one(g) for name, g in targets_by_name.items()}
        generated = {name: [r["converted"] for r in self.convert(g, name, bank)] for name, g in groups.items()}
        return ms.stats(groups), ms.stats(generated)

    def convert(self, sources: Sequence, targets, bank: StyleBank = None, style_mix: float = 1.0, recons: bool = False,
                postfilter=None) -> list:
        """sources: list of [80, L] arrays / tensors.  With a `bank`, targets is one of its names or one name per source;
        without one, targets is a mel or a list of mels that form the one style group of this call.
        -> per source {"converted": [80, L]} — content of the source, style (1 - style_mix) x the source's own mean style +
        style_mix x the target group's, post-net applied, clamped to [0, 1], exactly L frames.  recons=True adds "recons"
        [80, L] (the source's own mean style, no post-net, no clamp: convert_mel's other decode) and "decoded" (the converted
        path before the post-net and the clamp).  postfilter: None, or (modspec, natural, generated, alpha[, max_gain_db]) — a
        ModSpec, the two ModSpecStats of `smoothing_stats` and a strength in [0, 1]: "converted" then goes, after the clamp,
        through modspec.postfilter with the statistics of its source's target name, and is clamped again by the overlap-add."""
        mix = float(style_mix)
        if not 0.0 <= mix <= 1.0:
            raise ValueError(f"convert: style_mix={style_mix} outside [0, 1]")
        sources = list(sources)
        if not sources:
            return []
        if bank is None:
            one = (torch.is_tensor(targets) or isinstance(targets, np.ndarray)) and targets.ndim == 2
            bank = self.style_bank({"target": [targets] if one else list(targets)})
            targets = "target"
        self.check_bank(bank)
        names = [targets] * len(sources) if isinstance(targets, str) else list(targets)
        if len(names) != len(sources):
            raise ValueError("convert: one target name, or one per source")
        trg = np.asarray([bank.index(n) for n in names], dtype=np.int32)
        nutt = len(sources)
        with self._eval():
            plan, packed = self.pack(sources)
            utt_d, win_d = plan["utt_d"], plan["win_d"]
            style, content = self.encode(mel_to_windows(packed, utt_d, win_d, self.T))
            u = plan["win"][:, 0]
            g_src = upload(u, self.device, np.int32)
            own_sums, own_counts = self.group_sums(style, g_src, nutt)
            sums = torch.cat([own_sums, upload(bank.sums, self.device, np.float64)])
            counts = torch.cat([own_counts, upload(bank.counts, self.device, np.int64)])
            counts_host = np.concatenate([own_counts.cpu().numpy(), bank.counts])
            g_trg = upload(np.where(u >= 0, nutt + trg[np.maximum(u, 0)], -1), self.device, np.int32)
            z = window_latents(content, sums, counts, g_src, g_trg, mix, self.S, counts_host)
            dec, post = self.decode(z)
            conv = windows_overlap_add(post, utt_d, win_d, self.window, plan["ld"], clamp=(0.0, 1.0))
            outs = {"converted": conv}
            if recons:
                outs["decoded"] = windows_overlap_add(dec, utt_d, win_d, self.window, plan["ld"])
                z0 = window_latents(content, sums, counts, g_src, g_src, 0.0, self.S, counts_host)
                outs["recons"] = windows_overlap_add(self.decode(z0)[0], utt_d, win_d, self.window, plan["ld"])
            res = [{k: v[:, col0:col0 + L].contiguous() for k, v in outs.items()} for col0, L, _, _ in plan["utt"]]
            if postfilter is not None:
                ms, natural, generated, alpha = postfilter[:4]
                for name in dict.fromkeys(names):
                    idx = [i for i, n in enumerate(names) if n == name]
                    for i, y in zip(idx, ms.postfilter([res[i]["converted"] for i in idx], (natural, name), (generated, name),
                                                       alpha, *postfilter[4:])):
                        res[i]["converted"] = y
        self.trainer._check_device_errors()
        return res


# ------------------------------------------------------------------------------------------------------- wav in, wav out
def list_wavs(paths: Sequence) -> list:
    """files as given, directories as their sorted **/*.wav"""
    out = []
    for p in paths:
        p = Path(p)
        out += sorted(p.glob("**/*.wav")) if p.is_dir() else [p]
    return out


def wavs_to_mels(paths: Sequence, fe, rs, report) -> list:
    """-> [(path, mel [80, M] float32 numpy, resampled sample count)] of the usable files; the others are reported
    (unreadable, empty, too short to resample, silent) and left out.  The corpus's own path: preprocess._run_batch."""
    from .preprocess import SAMPLE_RATE, _run_batch, read_wav, resample_lengths
    good = []
    for p in paths:
        try:
            wav, sr = read_wav(p, 600.0)
        except (OSError, ValueError) as e:
            report(f"skipped {p}: {e}")
            continue
        if wav.shape[0] == 0:
            report(f"skipped {p}: empty")
        elif sr != SAMPLE_RATE and resample_lengths(wav.shape[0], sr)[0] < 1:
            report(f"skipped {p}: too short to resample ({wav.shape[0]} samples at {sr} Hz)")
        else:
            n16 = wav.shape[0] if sr == SAMPLE_RATE else int(resample_lengths(wav.shape[0], sr)[1])
            good.append((p, wav, sr, n16))
    out = []
    if good:
        for (p, _, _, n16), (mel, why) in zip(good, _run_batch(fe, rs, [g[1] for g in good], [g[2] for g in good])):
            if why:
                report(f"skipped {p}: {why}")
            else:
                out.append((p, mel, n16))
    return out


def load_run(log_dir, device, use_ema=False, use_best=False):
    """The trainer of a `python -m dvae_amd.train` run: built from <log_dir>/config.json, weights from <log_dir>/checkpoints
    (the last iterate, its average, or the one best.json names) -> (trainer, checkpoint file name)."""
    from .model.disentangled_vae import ConvolutionalMulVAE
    from .probe import checkpoint_files
    log_dir = Path(log_dir)
    cfg_path = log_dir.joinpath("config.json")
    if not cfg_path.is_file():
        raise SystemExit(f"convert: {cfg_path} is missing: --log_dir must be the --log_dir of a python -m dvae_amd.train run")
    cfg = json.loads(cfg_path.read_text())
    ckpt_dir = log_dir.joinpath("checkpoints")
    files = checkpoint_files(ckpt_dir)
    if not files:
        raise SystemExit(f"convert: no checkpoint under {ckpt_dir}: train the model first")
    latent = int(cfg.get("latent_size", 32))
    vsc = ConvolutionalMulVAE(cfg.get("dataset", "VCTK"), int(cfg.get("samples_length", 64)), N_MEL, latent,
                              float(cfg.get("lr", 1e-3)), float(cfg.get("alpha", 0.01)), int(cfg.get("log_interval", 500)),
                              bool(cfg.get("normalize", False)), speaker_size=int(cfg.get("speaker_size", 4)), device=device,
                              latent_dim=latent, beta=float(cfg.get("beta_cof", 0.1)), batch_size=int(cfg.get("batch_size", 2)),
                              mse_cof=float(cfg.get("mse_cof", 10)), kl_cof=float(cfg.get("kl_cof", 10)),
                              style_cof=float(cfg.get("style_cof", 0.1)))
    quiet = lambda *_: None
    if use_best:
        from .train import load_best
        return vsc, load_best(vsc, str(ckpt_dir), quiet)["weights"]
    try:
        vsc.load_last_model(str(ckpt_dir), logging_func=quiet, use_ema=use_ema)
    except FileNotFoundError as e:
        raise SystemExit(f"convert: --use-ema: {e}")
    last = max(files, key=lambda f: int(Path(f).stem.split("_")[2]))
    return vsc, os.path.basename(last[:-4] + ".ema.pth" if use_ema else last)


def _parse(argv):
    p = argparse.ArgumentParser(prog="python -m dvae_amd.convert",
                                description="Convert whole utterances, wav to wav, with the model of a training run.")
    p.add_argument("--log_dir", type=Path, required=True, help="the run: config.json and checkpoints/ of train.py")
    p.add_argument("--source", nargs="+", required=True, help=".wav files, or directories of them: what is said")
    p.add_argument("--target", nargs="+", required=True, help=".wav files, or directories of them: ONE style group, the voice")
    p.add_argument("-o", "--out", type=Path, default=None, help="output directory (default <log_dir>/generation/wav)")
    p.add_argument("--hop", type=int, default=None, help="frames between windows (default T / 2)")
    p.add_argument("--style-mix", type=float, default=1.0, help="1: the target's style, 0: the source's own, between: a blend")
    p.add_argument("--griffin-lim-iters", type=int, default=32)
    p.add_argument("--use-ema", action="store_true", default=False, help="voice the averaged weights")
    p.add_argument("--use-best", action="store_true", default=False, help="voice the checkpoint checkpoints/best.json names")
    p.add_argument("--batch", type=int, default=32, help="windows per forward (one fixed shape)")
    p.add_argument("--seed", type=int, default=1, help="seed of the Griffin-Lim start phase")
    p.add_argument("--ms-postfilter", type=float, default=None, metavar="ALPHA",
                   help="modulation-spectrum postfilter of strength ALPHA in (0, 1] against over-smoothing: statistics from the "
                        "--target files and from their own conversions (off by default)")
    p.add_argument("--ms-window", type=int, default=64, metavar="D", help="frames per postfilter window (even, 8 ... 128)")
    p.add_argument("--ms-max-gain-db", type=float, default=12.0, metavar="G",
                   help="largest gain or attenuation of a modulation component (a safeguard, not a measured optimum)")
    return p.parse_args(argv)


def main(argv=None) -> int:
    args = _parse(sys.argv[1:] if argv is None else argv)
    report = lambda msg: print(f"convert: {msg}", file=sys.stderr)
    if args.use_ema and args.use_best:
        report("--use-ema and --use-best exclude each other")
        return 2
    if not 0.0 <= args.style_mix <= 1.0:
        report(f"--style-mix {args.style_mix} outside [0, 1]")
        return 2
    if args.ms_postfilter is not None:
        from .modspec import check_window
        if not 0.0 < args.ms_postfilter <= 1.0:
            report(f"--ms-postfilter {args.ms_postfilter} outside (0, 1]")
            return 2
        if not args.ms_max_gain_db > 0.0:
            report(f"--ms-max-gain-db {args.ms_max_gain_db} must be positive")
            return 2
        try:
            check_window(args.ms_window)
        except ValueError as e:
            report(f"--ms-window: {e}")
            return 2
    if not torch.cuda.is_available():
        report("no GPU: conversion runs on the HIP path only")
        return 2
    from .frontend import MelFrontend, MelInverter
    from .preprocess import Resampler
    from .train import write_wav
    device = torch.device("cuda", torch.cuda.current_device())
    vsc, ckpt = load_run(args.log_dir, device, args.use_ema, args.use_best)
    try:
        conv = Converter(vsc, hop=args.hop, batch=args.batch, checkpoint=ckpt)
    except ValueError as e:
        report(str(e))
        return 2
    fe, rs = MelFrontend(device), Resampler(device)
    inv = MelInverter(device=device)
    targets = wavs_to_mels(list_wavs(args.target), fe, rs, report)
    if not targets:
        report("no usable --target file")
        return 1
    sources = [s for s in wavs_to_mels(list_wavs(args.source), fe, rs, report)]
    short = [s for s in sources if s[1].shape[1] < inv.min_frames]
    for p, mel, _ in short:
        report(f"skipped {p}: {mel.shape[1]} frames, the vocoder needs {inv.min_frames}")
    sources = [s for s in sources if s[1].shape[1] >= inv.min_frames]
    if not sources:
        report("no usable --source file")
        return 1
    out_dir = args.out or args.log_dir.joinpath("generation", "wav")
    out_dir.mkdir(parents=True, exist_ok=True)
    bank = conv.style_bank({"target": [t[1] for t in targets]})
    postfilter = None
    if args.ms_postfilter is not None:
        from .modspec import ModSpec
        ms = ModSpec(device, args.ms_window)
        natural, generated = conv.smoothing_stats({"target": [t[1] for t in targets]}, bank, ms)
        if natural.windows[0] < 1:
            report(f"--ms-postfilter: no --target file has {ms.D} frames: no statistics to filter towards")
            return 1
        postfilter = (ms, natural, generated, args.ms_postfilter, args.ms_max_gain_db)
    res = conv.convert([s[1] for s in sources], "target", bank, style_mix=args.style_mix, postfilter=postfilter)
    gen = torch.Generator(device=device)
    gen.manual_seed(args.seed)
    wavs = inv.waveform_batch([r["converted"] for r in res], n_iter=args.griffin_lim_iters, generator=gen)
    for (p, _, n16), r, w in zip(sources, res, wavs):
        stem = Path(p).stem
        np.save(out_dir.joinpath(f"convert_{stem}.npy"), r["converted"].cpu().numpy())
        write_wav(str(out_dir.joinpath(f"convert_{stem}.wav")), w[:n16].cpu().numpy(), inv.sr)
        print(f"wrote {out_dir.joinpath(f'convert_{stem}.wav')}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
