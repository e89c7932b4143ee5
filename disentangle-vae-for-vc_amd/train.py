"""CLI mirror of the reference's train.py for the training path (flags at /root/reference/train.py:15-46,65-71).

    python -m dvae_amd.train --train true --dataset_fp=<root> --batch-size=8 --latent-size=32 --speaker_size=4 \\
        --lr=1e-4 --epochs=10 --report-interval=5 --mse_cof=10 --kl_cof=10 --log_dir=./results

Kept flags: --batch-size --latent-size --speaker_size --lr --epochs --report-interval --mse_cof --kl_cof --seed
--dataset_fp --log_dir --train --samples_length (honoured here; the reference parses it but hard-codes 64,
train.py:53).  Parsed-and-ignored flags of the reference (--hidden-size --alpha --normalize --beta_cof --style_cof
--sample-size --no-cuda --do-not-resume --log-interval) are accepted for command-line compatibility.
--ema-decay F (new): an exponential moving average of the weights, kept on the device inside the step (optim.FlatAdam.set_ema)
and written as <name>_<epoch>.ema.pth next to every checkpoint; --use-ema makes --convert voice it.
--val-fraction F / --val-speakers a,b (new): a held-out part of the corpus that training never sees (data.split_corpus, fixed by
--val-seed and written to <log_dir>/val_split.json), the eight loss terms on it every --val-interval epochs (last iterate and,
with --ema-decay, the average: Val/... and Val EMA/... in scalars.jsonl, per speaker in <log_dir>/val.json) and
checkpoints/best.json naming the checkpoint with the lowest Val/Loss; --use-best makes --convert voice that one.
--kl-schedule {constant,linear,cyclical,double} / --free-bits F (new, opt-in): KL annealing and per-dimension free bits on the
training loss, on the device inside the replayed step (ConvolutionalMulVAE.set_kl_schedule, kl_schedule.py); KL/... in
scalars.jsonl, <log_dir>/kl_dims.json; the schedule rides in the .opt sidecar and a resume continues it.
--adv-weight F (new, opt-in): a speaker classifier on the content means, trained inside the replayed step, whose gradient
reaches the encoder reversed and scaled by F (ConvolutionalMulVAE.set_speaker_adversary, adversary.py; 0: it only monitors);
--adv-hidden, --adv-lr, --adv-warmup-steps; Adv/... in scalars.jsonl; it is checkpointed as <name>_<epoch>.adv.pth beside the
.pth, and a resume continues it (without the flags: with the saved configuration).
--tc-weight F [--shared-weight F] [--factor-warmup-steps N] (new, opt-in): the beta-TCVAE penalty on the minibatch of every
training step, inside the replayed step (ConvolutionalMulVAE.set_factor_penalty, csrc/factor.hip): F times the total correlation
inside the style and inside the content block, --shared-weight times the information the two blocks share; --tc-weight 0 alone
only monitors; Factor/... in scalars.jsonl; the configuration rides in the .opt sidecar and a resume continues it.
--ms-loss-weight F [--gv-loss-weight F] [--ms-loss-window D] [--ms-loss-floor F] [--ms-loss-warmup-steps N] (new, opt-in): the
modulation-spectrum and global-variance loss on rec_hat of every training step, inside the replayed step
(ConvolutionalMulVAE.set_smoothing_penalty, csrc/msloss.hip): F times the mean squared distance between the log modulation spectra
of the reconstruction and of its input, --gv-loss-weight times that between their log global variances; --ms-loss-weight 0 alone
only monitors; Smooth/... in scalars.jsonl; the configuration rides in the .opt sidecar and a resume continues it.
--convert (reference variational_base_vae.py:243-330, minus plots): the first --convert-count sorted utterances of
--src_spk, each with a random utterance of --trg_spk (seeded by --seed), through `convert_mel`; the converted mels are
voiced by the GPU Griffin-Lim inverse of the mel front-end (frontend.MelInverter, --griffin-lim-iters) instead of the
reference's WaveNet, whose code and weights are not part of the reference, and written to
<log_dir>/generation/<src>_to_<trg>/convert_<src>_to_<trg>_<utt>.wav (16 kHz mono PCM-16) with the source, reconstructed
and converted mels as .npy.
--convert --overlap HOP (new, opt-in): the same files through convert.Converter — every source whole, covered by windows HOP
frames apart and cross-faded on the device, exactly its own frame count, in the mean style of the first --trg-utts sorted
utterances of --trg_spk (all by default), --style-mix blending it with the source's own; the same file names.

Data parallel (new; the reference is single-device, train.py:49-58): started as one of WORLD_SIZE > 1 ranks —
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 -m dvae_amd.train ...` or with
`--gpus N` (this process then only launches N rank processes before anything touches the GPU) — every rank takes
LOCAL_RANK's GPU, joins the RCCL group, receives rank 0's weights, attaches ddp.GradReducer (bucketed all-reduce
overlapped with backward, 1/world inside Adam) and feeds from its shard of the device-resident corpus
(data.GpuPairLoader(rank=, world_size=): same epoch permutation on every rank, pairs rank, rank + world, ...).
--batch-size stays the PER-GPU batch (weak scaling).  Rank 0 writes checkpoints and logs.
"""
import argparse
import json
import os
import sys

import torch
from torch.utils.data import DataLoader


def get_parse():
    p = argparse.ArgumentParser()
    p.add_argument("--batch-size", type=int, default=2)
    p.add_argument("--hidden-size", type=str, default="400")
    p.add_argument("--speaker_size", type=int, default=4)
    p.add_argument("--latent-size", type=int, default=32)
    p.add_argument("--lr", default=1e-3, type=float)
    p.add_argument("--epochs", type=int, default=11)
    p.add_argument("--no-cuda", action="store_true", default=False)
    p.add_argument("--dataset", default="VCTK")
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--log-interval", type=int, default=500)
    p.add_argument("--report-interval", type=int, default=11)
    p.add_argument("--sample-size", type=int, default=64)
    p.add_argument("--do-not-resume", action="store_true", default=False)
    p.add_argument("--normalize", action="store_true", default=False)
    p.add_argument("--beta_cof", default=0.1, type=float)
    p.add_argument("--mse_cof", default=10, type=float)
    p.add_argument("--kl_cof", default=10, type=float)
    p.add_argument("--style_cof", default=0.1, type=float)
    p.add_argument("--samples_length", default=64, type=int)
    p.add_argument("--alpha", default=0.01, type=float)
    p.add_argument("--dataset_fp", default="/root/VCTK-Corpus/Autovc-known-speakers", type=str)
    p.add_argument("--log_dir", default="./results", type=str)
    p.add_argument("--train", type=bool, default=False)
    p.add_argument("--convert", type=bool, default=False)
    p.add_argument("--src_spk", default="VCTK-Corpus_wav16_p225", type=str)
    p.add_argument("--trg_spk", default="VCTK-Corpus_wav16_p226", type=str)
    p.add_argument("--convert-count", type=int, default=2, help="--convert: the first N sorted utterances of --src_spk")
    p.add_argument("--griffin-lim-iters", type=int, default=32, help="--convert: Griffin-Lim iterations of the vocoder")
    p.add_argument("--graph", type=int, default=1, help="replay the step from a hipGraph (fixed batch shape)")
    p.add_argument("--gpus", type=int, default=0,
                   help="data-parallel ranks on this node; > 1 without WORLD_SIZE in the environment: launch them")
    p.add_argument("--gpu-loader", type=int, default=-1,
                   help="1: device-resident corpus + HIP gather/crop (data.GpuPairLoader); 0: the reference's DataLoader; "
                        "-1: the GPU loader when data parallel, the DataLoader otherwise")
    p.add_argument("--clip-grad-norm", type=float, default=0.0,
                   help="clip the global L2 norm of the gradient to this value and skip steps whose gradient is not finite, "
                        "on the device inside the step (0: off)")
    p.add_argument("--log-grad-norm", action="store_true", default=False,
                   help="measure the gradient norm and keep the non-finite guard without clipping (max_norm = inf); "
                        "scalars.jsonl gains the Grad/... keys either way")
    p.add_argument("--ema-decay", type=float, default=0.0,
                   help="keep an exponential moving average of the weights with this decay (0 < F < 1; warm-up "
                        "min(F, (1 + k) / (10 + k))), on the device inside the step, and write it next to every checkpoint as "
                        "<name>_<epoch>.ema.pth (0: off)")
    p.add_argument("--use-ema", action="store_true", default=False,
                   help="--convert: voice the averaged weights (<name>_<epoch>.ema.pth) instead of the last iterate")
    p.add_argument("--val-fraction", type=float, default=0.0,
                   help="hold this fraction of every speaker's utterances out of training (0 <= F < 0.5) and report the "
                        "loss terms on them every --val-interval epochs (0: off)")
    p.add_argument("--val-speakers", type=str, default="", help="comma-separated speakers held out whole")
    p.add_argument("--val-seed", type=int, default=0, help="seed of the split and of the validation pass's style noise")
    p.add_argument("--val-interval", type=int, default=1, help="validate every N epochs (and at every checkpoint)")
    p.add_argument("--use-best", action="store_true", default=False,
                   help="--convert: voice the checkpoint that checkpoints/best.json names (lowest Val/Loss)")
    p.add_argument("--overlap", type=int, default=0,
                   help="--convert: whole utterances through windows HOP frames apart, cross-faded (convert.Converter), with the "
                        "mean style of the target speaker's utterances (0: the reference's disjoint chunks)")
    p.add_argument("--trg-utts", type=int, default=0,
                   help="--convert --overlap: the style comes from the first N sorted utterances of --trg_spk (0: all)")
    p.add_argument("--style-mix", type=float, default=1.0,
                   help="--convert --overlap: 1 the target's style, 0 the source's own mean style, between: a blend")
    p.add_argument("--kl-schedule", choices=("constant", "linear", "cyclical", "double"), default=None,
                   help="anneal the KL weight of the training loss on the device, inside the replayed step: constant (kl_cof), "
                        "linear (--kl-start to kl_cof over --kl-warmup-steps steps), cyclical (the same steps cut into "
                        "--kl-cycles cycles, each ramping over its first --kl-ratio), double (--kl-start, doubled every "
                        "epoch, capped at kl_cof: the reference's update_kl).  Validation keeps kl_cof.  Default: off")
    p.add_argument("--kl-start", type=float, default=0.0, help="--kl-schedule: the weight the ramp starts from")
    p.add_argument("--kl-warmup-steps", type=int, default=0, help="--kl-schedule linear / cyclical: optimiser steps of the ramp(s)")
    p.add_argument("--kl-cycles", type=int, default=4, help="--kl-schedule cyclical: number of cycles")
    p.add_argument("--kl-ratio", type=float, default=0.5, help="--kl-schedule cyclical: the rising part of a cycle")
    p.add_argument("--free-bits", type=float, default=None,
                   help="nats every latent dimension may spend unpenalised (batch-mean KL per dimension, Kingma et al. 2016); "
                        "without --kl-schedule it implies constant")
    p.add_argument("--free-bits-style", type=float, default=None, help="--free-bits of the style dimensions only")
    p.add_argument("--free-bits-content", type=float, default=None, help="--free-bits of the content dimensions only")
    p.add_argument("--adv-weight", type=float, default=None,
                   help="train a speaker classifier on the content means inside the step and send its gradient to the encoder "
                        "reversed, scaled by this weight (0: the classifier learns, the model is untouched: a leakage monitor). "
                        "Default: off")
    p.add_argument("--adv-hidden", type=int, default=256, help="--adv-weight: hidden width of the classifier (a multiple of 64)")
    p.add_argument("--adv-lr", type=float, default=1e-3, help="--adv-weight: learning rate of the classifier's own Adam")
    p.add_argument("--adv-warmup-steps", type=int, default=0,
                   help="--adv-weight: the weight rises linearly from 0 over this many optimiser steps")
    p.add_argument("--tc-weight", type=float, default=None,
                   help="penalise the total correlation inside the style and inside the content block on the minibatch of every "
                        "training step, with this weight, in nats per row (0 without --shared-weight: the statistics are "
                        "computed, the model is untouched: a monitor).  Default: off")
    p.add_argument("--shared-weight", type=float, default=None,
                   help="penalise the information the style and the content block share, with this weight; alone it implies "
                        "--tc-weight 0")
    p.add_argument("--factor-warmup-steps", type=int, default=0,
                   help="--tc-weight / --shared-weight: both weights rise linearly from 0 over this many optimiser steps")
    p.add_argument("--ms-loss-weight", type=float, default=None,
                   help="penalise the mean squared distance between the log modulation spectra of rec_hat and of the input it "
                        "reconstructs on every training step, with this weight, in nats^2 (0 without --gv-loss-weight: the "
                        "statistics are computed, the model is untouched: a monitor).  Default: off")
    p.add_argument("--gv-loss-weight", type=float, default=None,
                   help="penalise the mean squared distance between their log global variances, with this weight; alone it "
                        "implies --ms-loss-weight 0")
    p.add_argument("--ms-loss-window", type=int, default=None,
                   help="--ms-loss-weight: frames of a window (even, 8 .. 128, a divisor of --samples_length; default min(64, T))")
    p.add_argument("--ms-loss-floor", type=float, default=0.003,
                   help="--ms-loss-weight / --gv-loss-weight: the ripple under which a logarithm stops following its argument "
                        "(0.003 = 0.3 dB of the normalised range; a setting, not a measured optimum)")
    p.add_argument("--ms-loss-warmup-steps", type=int, default=0,
                   help="--ms-loss-weight / --gv-loss-weight: both weights rise linearly from 0 over this many optimiser steps")
    return p


SMOOTH_KEYS = ("ms_loss_weight", "gv_loss_weight", "ms_loss_window", "ms_loss_floor", "ms_loss_warmup_steps")
FACTOR_KEYS = ("tc_weight", "shared_weight", "factor_warmup_steps")
ADV_KEYS = ("adv_weight", "adv_hidden", "adv_lr", "adv_warmup_steps")
KL_KEYS = ("kl_schedule", "kl_start", "kl_warmup_steps", "kl_cycles", "kl_ratio", "free_bits", "free_bits_style",
           "free_bits_content")


def kl_schedule_args(args):
    """(kind, keyword arguments) of ConvolutionalMulVAE.set_kl_schedule from the command line; kind None: off."""
    style = args.free_bits_style if args.free_bits_style is not None else args.free_bits
    content = args.free_bits_content if args.free_bits_content is not None else args.free_bits
    fb = None if style is None and content is None else (style or 0.0, content or 0.0)
    kind = args.kl_schedule or ("constant" if fb is not None else None)
    return kind, dict(start=args.kl_start, steps=args.kl_warmup_steps, cycles=args.kl_cycles, ratio=args.kl_ratio,
                      free_bits=fb)


def get_dataset(dataset_fp, batch_size, samples_length=64, seed=None, exclude=None):
    from .data import SpeechDatasetGVAE
    ds = SpeechDatasetGVAE(dataset_fp, samples_length=samples_length, seed=seed, exclude=exclude)
    # drop_last keeps the batch shape fixed (hipGraph replay); the reference uses drop_last=False (train.py:55-56)
    return DataLoader(ds, batch_size=batch_size, pin_memory=True, shuffle=True, drop_last=True), ds


def launch_ranks(n, argv):
    """--gpus n without a rendezvous in the environment: n fresh rank processes of this module, started before anything
    here touches the GPU; returns the first non-zero exit code (0 if all ranks succeeded)."""
    import socket
    import subprocess
    import sys
    import time
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
        procs.append(subprocess.Popen([sys.executable, "-c", "import dvae_amd.train as t, sys; t.main(sys.argv[1:])"]
                                      + list(argv), env=env))
    rc, live = 0, set(range(n))
    while live:
        for r in sorted(live):
            code = procs[r].poll()
            if code is None:
                continue
            live.discard(r)
            if code != 0 and rc == 0:
                rc = code
                for q in live:
                    procs[q].terminate()          # exactly the PIDs started above
        time.sleep(0.05)
    return rc if rc >= 0 else 128 - rc


def setup_data_parallel(vsc, seed):
    """Join the process group (RCCL; DVAE_DIST_BACKEND overrides for functional checks), take rank 0's weights and
    BatchNorm buffers, attach the gradient reducer.  Returns (rank, world)."""
    import torch.distributed as dist
    from . import ddp
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29519")
        backend = os.environ.get("DVAE_DIST_BACKEND", "nccl")
        if os.environ.get("DVAE_RCCL_MAX_CHANNELS"):
            os.environ["NCCL_MAX_NCHANNELS"] = os.environ["DVAE_RCCL_MAX_CHANNELS"]
        kw = {"device_id": torch.device(vsc.device)} if backend == "nccl" else {}
        dist.init_process_group(backend, rank=rank, world_size=world, **kw)
    opt = vsc.optimizer
    ddp.broadcast_parameters(opt.flat_p, list(vsc.model.buffers()))
    red = ddp.GradReducer(opt.flat_g, opt.names, opt.params, opt.offsets,
                          mode=os.environ.get("DVAE_DDP_MODE", "all_reduce"),     # "rs_ag": reduce-scatter + sharded Adam
                          issue=os.environ.get("DVAE_DDP_ISSUE", "finish"))       # default: collectives after backward (nothing beside the W_hh-resident recurrences, the variant bench.py measures first and reports as the headline); "hook": issued from the backward hooks (overlap)
    red.force = os.environ.get("DVAE_FORCE_DDP", "0") == "1"      # issue the collectives with one rank too (tests)
    vsc.attach_reducer(red)
    return rank, world


def _abort_process_group():
    """Best effort, never blocks: abort the communicators of a failing rank (no collective, no barrier)."""
    try:
        import torch.distributed as dist
        if not dist.is_initialized():
            return
        pg = dist.distributed_c10d._get_default_group()
        be = None
        try:
            be = pg._get_backend(torch.device("cuda"))
        except Exception:
            pass
        for obj in (be, pg):
            for name in ("abort", "_abort", "_shutdown"):
                fn = getattr(obj, name, None)
                if callable(fn):
                    try:
                        fn()
                        return
                    except Exception:
                        pass
    except Exception:
        pass


def utterance_id(path: str) -> str:
    """reference variational_base_vae.py:275: `<anything>_<utt>_<suffix>.npy` -> <utt>"""
    parts = os.path.basename(path).split(".")[0].split("_")
    return parts[-2] if len(parts) >= 2 else parts[0]


def write_wav(path: str, wav, sample_rate: int = 16000):
    """mono PCM-16 .wav (soundfile's default subtype for .wav), samples clipped to [-1, 1]"""
    import wave

    import numpy as np
    x = np.clip(np.asarray(wav, dtype=np.float64), -1.0, 1.0)
    pcm = np.round(x * 32767.0).astype("<i2")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sample_rate)
        w.writeframes(pcm.tobytes())


def load_best(vsc, checkpoints_path, logging_func=print):
    """--use-best: the weights that <checkpoints>/best.json names (run_training writes it while validation is on)."""
    path = os.path.join(checkpoints_path, "best.json")
    if not os.path.exists(path):
        raise SystemExit(f"--use-best: {path} is missing (train with --val-fraction / --val-speakers)")
    with open(path) as fp:
        best = json.load(fp)
    weights = os.path.join(checkpoints_path, best["weights"])
    if not os.path.exists(weights):
        raise SystemExit(f"--use-best: {path} names {best['weights']}, which is missing")
    vsc.model.load_state_dict(torch.load(weights, map_location=vsc.device))
    logging_func(f"Loading the best checkpoint {best['weights']} (epoch {best['epoch']}, Val/Loss {best['Val/Loss']:.4f})...")
    return best


def held_out_split(args, rank=0):
    """(held, excluded) of --val-fraction / --val-speakers, or (None, None) when neither is given.  The first run writes
    <log_dir>/val_split.json; a later run on the same <log_dir> reads it, and exits if its flags ask for another split."""
    from .data import excluded_files, read_val_split, split_corpus, write_val_split
    speakers = tuple(s for s in args.val_speakers.split(",") if s)
    path = os.path.join(args.log_dir, "val_split.json")
    # (the other ranks of a data-parallel run compute the same split from the same flags: rank 0 may still be writing)
    if rank == 0 and os.path.exists(path) and not args.do_not_resume:
        return read_val_split(path, args.dataset_fp, args.val_fraction, speakers, args.val_seed)
    if args.val_fraction == 0.0 and not speakers:
        return None, None
    try:
        held = split_corpus(args.dataset_fp, args.val_fraction, speakers, args.val_seed)
        excluded = excluded_files(args.dataset_fp, args.val_fraction, speakers, args.val_seed)
    except ValueError as e:
        raise SystemExit(f"--val-fraction / --val-speakers: {e}")
    if not held:
        raise SystemExit("--val-fraction / --val-speakers: nothing is held out (two files per speaker at the least)")
    if rank == 0:
        os.makedirs(args.log_dir, exist_ok=True)
        write_val_split(path, args.dataset_fp, held, excluded, args.val_fraction, speakers, args.val_seed)
    return held, excluded


def convert(vsc, args, logging_func=print):
    """--convert: reference voice_conversion_mel (variational_base_vae.py:243-330) with the Griffin-Lim vocoder"""
    from glob import glob

    import numpy as np

    from .frontend import MelInverter
    src, trg = args.src_spk, args.trg_spk
    save_dir = os.path.join(args.log_dir, "generation", f"{src}_to_{trg}")
    os.makedirs(save_dir, exist_ok=True)
    if getattr(args, "use_best", False):
        load_best(vsc, os.path.join(args.log_dir, "checkpoints"), logging_func)
    else:
        try:
            vsc.load_last_model(os.path.join(args.log_dir, "checkpoints"), logging_func=logging_func,
                                use_ema=bool(getattr(args, "use_ema", False)))
        except FileNotFoundError as e:
            raise SystemExit(f"--use-ema: {e}")
    sources = sorted(glob(os.path.join(args.dataset_fp, src, "*.npy")))[:args.convert_count]
    targets = sorted(glob(os.path.join(args.dataset_fp, trg, "*.npy")))
    if not sources or not targets:
        raise SystemExit(f"--convert: no .npy utterances under {args.dataset_fp}/{src} or {args.dataset_fp}/{trg}")
    if getattr(args, "overlap", 0):
        return convert_overlapped(vsc, args, sources, targets, save_dir, logging_func)
    rng = np.random.RandomState(args.seed)
    names, converted = [], []
    for fp in sources:
        t = targets[rng.randint(len(targets))]
        utt = utterance_id(fp)
        logging_func(f"convert utterance: {utt} from --->{src} to --->{trg}")
        out = vsc.convert_mel(np.load(fp), np.load(t))
        np.save(os.path.join(save_dir, f"source_{src}_{utt}.npy"), out["source"].cpu().numpy())
        np.save(os.path.join(save_dir, f"recons_{src}_{utt}.npy"), out["recons"].cpu().numpy())
        np.save(os.path.join(save_dir, f"convert_{src}_to_{trg}_{utt}.npy"), out["converted"].cpu().numpy())
        names.append(f"convert_{src}_to_{trg}_{utt}.wav")
        converted.append(out["converted"])
    inv = MelInverter(device=vsc.device)
    gen = torch.Generator(device=vsc.device)
    gen.manual_seed(args.seed)
    wavs = inv.waveform_batch(converted, n_iter=args.griffin_lim_iters, generator=gen)
    for name, w in zip(names, wavs):
        write_wav(os.path.join(save_dir, name), w.cpu().numpy(), inv.sr)
        logging_func(f"wrote {os.path.join(save_dir, name)}")
    return [os.path.join(save_dir, n) for n in names]


def convert_overlapped(vsc, args, sources, targets, save_dir, logging_func=print):
    """--convert --overlap HOP: the corpus files through convert.Converter — every source whole, exactly its own frame count,
    in the mean style of the first --trg-utts target utterances; file names as the chunk path writes them."""
    import numpy as np

    from .convert import Converter
    from .frontend import MelInverter
    src, trg = args.src_spk, args.trg_spk
    if not 0.0 <= args.style_mix <= 1.0:
        raise SystemExit(f"--style-mix {args.style_mix}: a weight in [0, 1]")
    try:
        conv = Converter(vsc, hop=args.overlap, batch=32)
    except ValueError as e:
        raise SystemExit(f"--overlap: {e}")
    if args.trg_utts > 0:
        targets = targets[:args.trg_utts]
    bank = conv.style_bank({trg: [np.load(t) for t in targets]})
    mels = [np.load(fp) for fp in sources]
    res = conv.convert(mels, trg, bank, style_mix=args.style_mix, recons=True)
    names = []
    for fp, mel, r in zip(sources, mels, res):
        utt = utterance_id(fp)
        logging_func(f"convert utterance: {utt} from --->{src} to --->{trg} ({len(targets)} target utterances, hop {conv.hop})")
        np.save(os.path.join(save_dir, f"source_{src}_{utt}.npy"), np.asarray(mel, dtype=np.float32))
        np.save(os.path.join(save_dir, f"recons_{src}_{utt}.npy"), r["recons"].cpu().numpy())
        np.save(os.path.join(save_dir, f"convert_{src}_to_{trg}_{utt}.npy"), r["converted"].cpu().numpy())
        names.append(f"convert_{src}_to_{trg}_{utt}.wav")
    inv = MelInverter(device=vsc.device)
    gen = torch.Generator(device=vsc.device)
    gen.manual_seed(args.seed)
    wavs = inv.waveform_batch([r["converted"] for r in res], n_iter=args.griffin_lim_iters, generator=gen)
    for name, w in zip(names, wavs):
        write_wav(os.path.join(save_dir, name), w.cpu().numpy(), inv.sr)
        logging_func(f"wrote {os.path.join(save_dir, name)}")
    return [os.path.join(save_dir, n) for n in names]


def main(argv=None):
    args = get_parse().parse_args(argv)
    if not 0.0 <= args.ema_decay < 1.0:
        raise SystemExit(f"--ema-decay {args.ema_decay}: a decay with 0 < F < 1, or 0 for off")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        import sys
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:] if argv is None else argv))
    if args.gpus and args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    from .model.disentangled_vae import ConvolutionalMulVAE
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    n_dev = torch.cuda.device_count()
    if world > 1:
        if world > n_dev and os.environ.get("DVAE_ALLOW_SHARED_GPU", "0") != "1":
            raise SystemExit(f"{world} ranks but {n_dev} visible GPU(s): one process per GPU")
        if world > n_dev:
            from . import ops
            ops.LSTM_PERSISTENT = False      # two persistent grids cannot both be resident on one GPU
        torch.cuda.set_device(local % max(1, n_dev))
    device = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed(args.seed + 7919 * rank)      # every rank its own reparameterisation-noise stream
    if rank == 0:
        os.makedirs(args.log_dir, exist_ok=True)
        cfg = dict(vars(args))
        val_keys = ("val_fraction", "val_speakers", "val_seed", "val_interval", "use_best")
        if all(cfg[k] == get_parse().get_default(k) for k in val_keys):
            for k in val_keys:      # none of the validation flags given: the file a run wrote before they existed
                del cfg[k]
        conv_keys = ("overlap", "trg_utts", "style_mix")
        if all(cfg[k] == get_parse().get_default(k) for k in conv_keys):
            for k in conv_keys:     # likewise the flags of the overlapped conversion
                del cfg[k]
        for keys in (KL_KEYS, ADV_KEYS, FACTOR_KEYS, SMOOTH_KEYS):      # likewise the flags of each feature of the train step
            if all(cfg[k] == get_parse().get_default(k) for k in keys):
                for k in keys:
                    del cfg[k]
        with open(os.path.join(args.log_dir, "config.json"), "w") as fp:
            json.dump(cfg, fp, indent=4)
    vsc = ConvolutionalMulVAE(args.dataset, args.samples_length, 80, args.latent_size, args.lr, args.alpha,
                              args.log_interval, args.normalize, speaker_size=args.speaker_size, device=device,
                              latent_dim=args.latent_size, beta=args.beta_cof, batch_size=args.batch_size,
                              mse_cof=args.mse_cof, kl_cof=args.kl_cof, style_cof=args.style_cof)
    if args.clip_grad_norm < 0:
        raise SystemExit(f"--clip-grad-norm {args.clip_grad_norm}: a positive norm, or 0 for off")
    if args.clip_grad_norm > 0 or args.log_grad_norm:
        vsc.optimizer.set_grad_clip(args.clip_grad_norm if args.clip_grad_norm > 0 else float("inf"))
    if args.ema_decay > 0:
        vsc.optimizer.set_ema(args.ema_decay)
    kl_kind, kl_kw = kl_schedule_args(args)
    if kl_kind is not None:
        try:
            vsc.set_kl_schedule(kl_kind, **kl_kw)
        except ValueError as e:
            raise SystemExit(f"--kl-schedule / --free-bits: {e}")
    if args.tc_weight is None and args.shared_weight is None and args.factor_warmup_steps != 0:
        raise SystemExit("--factor-warmup-steps configures --tc-weight / --shared-weight: give one of them too (a resume "
                         "without any of the three restores the saved configuration)")
    if args.tc_weight is not None or args.shared_weight is not None:
        if not args.train:
            raise SystemExit("--tc-weight / --shared-weight: the factor penalty belongs to training (--train true)")
        try:
            vsc.set_factor_penalty(args.tc_weight if args.tc_weight is not None else 0.0,
                                   args.shared_weight if args.shared_weight is not None else 0.0,
                                   warmup_steps=args.factor_warmup_steps)
        except ValueError as e:
            raise SystemExit(f"--tc-weight / --shared-weight: {e}")
    smooth_on = args.ms_loss_weight is not None or args.gv_loss_weight is not None
    if not smooth_on and any(getattr(args, k) != get_parse().get_default(k) for k in SMOOTH_KEYS[2:]):
        raise SystemExit("--ms-loss-window / --ms-loss-floor / --ms-loss-warmup-steps configure --ms-loss-weight / "
                         "--gv-loss-weight: give one of them too (a resume without any of the five restores the saved "
                         "configuration)")
    if smooth_on:
        if not args.train:
            raise SystemExit("--ms-loss-weight / --gv-loss-weight: the smoothing penalty belongs to training (--train true)")
        try:
            vsc.set_smoothing_penalty(args.ms_loss_weight if args.ms_loss_weight is not None else 0.0,
                                      args.gv_loss_weight if args.gv_loss_weight is not None else 0.0,
                                      window=args.ms_loss_window, floor=args.ms_loss_floor,
                                      warmup_steps=args.ms_loss_warmup_steps)
        except ValueError as e:
            raise SystemExit(f"--ms-loss-weight / --gv-loss-weight: {e}")
    dp = world > 1 or os.environ.get("DVAE_FORCE_DDP", "0") == "1"
    if dp:
        setup_data_parallel(vsc, args.seed)
    use_gpu_loader = args.gpu_loader == 1 or (args.gpu_loader < 0 and dp)
    held, excluded = held_out_split(args, rank) if args.train else (None, None)
    val_kw = {}
    if held is not None:
        vsc.val_seed = args.val_seed
        if rank == 0:       # only rank 0 validates, as only rank 0 runs estimate_trained_model
            from .data import HeldOutPairs, SpeechDatasetGVAE as _DS
            ids = _DS.list_speakers(args.dataset_fp)
            val_kw = {"val_pairs": HeldOutPairs(held, args.samples_length, ids, device), "val_interval": args.val_interval}
    if use_gpu_loader:
        from .data import GpuPairLoader, SpeechDatasetGVAE
        ds = SpeechDatasetGVAE(args.dataset_fp, samples_length=args.samples_length, seed=args.seed, exclude=excluded)
        loader = GpuPairLoader(ds, args.batch_size, device=device, seed=args.seed, rank=rank, world_size=world)
    else:
        if world > 1:
            raise SystemExit("--gpu-loader 0 has no sharding: data-parallel runs feed from data.GpuPairLoader")
        loader, _ = get_dataset(args.dataset_fp, args.batch_size, args.samples_length, seed=args.seed, exclude=excluded)
    if args.adv_weight is None and any(getattr(args, k) != get_parse().get_default(k) for k in ADV_KEYS):
        raise SystemExit("--adv-hidden / --adv-lr / --adv-warmup-steps configure --adv-weight: give it too (a resume without "
                         "any of the four restores the saved configuration)")
    if args.adv_weight is not None:
        if not args.train:
            raise SystemExit("--adv-weight: the speaker adversary belongs to training (--train true)")
        try:
            vsc.set_speaker_adversary(args.adv_weight, n_speakers=len(loader.dataset.speaker_ids), hidden=args.adv_hidden,
                                      lr=args.adv_lr, warmup_steps=args.adv_warmup_steps, seed=args.seed)
        except ValueError as e:
            raise SystemExit(f"--adv-weight: {e}")
    if args.graph:
        vsc.enable_graph(True)     # with a reducer attached the step still runs eagerly unless DVAE_DDP_GRAPH=1
    hist = None
    try:
        # failure injection of tests/test_hip_train_cli.py (a rank that dies while its peers are in a collective): only in
        # an explicit test mode, never from a stray variable in a production environment
        if os.environ.get("DVAE_TEST_MODE") == "1" and os.environ.get("DVAE_TEST_FAIL_RANK") == str(rank):
            raise RuntimeError(f"injected failure on rank {rank} (DVAE_TEST_MODE / DVAE_TEST_FAIL_RANK)")
        if args.train:
            hist = vsc.run_training(loader, loader, args.epochs, args.report_interval, args.sample_size,
                                    reload_model=not args.do_not_resume,
                                    checkpoints_path=os.path.join(args.log_dir, "checkpoints"),
                                    images_path=os.path.join(args.log_dir, "images"),
                                    logs_path=os.path.join(args.log_dir, "logs"),
                                    estimation_dir=os.path.join(args.log_dir, "images", "estimation"), **val_kw)
        if args.convert and rank == 0:
            convert(vsc, args)
    except BaseException:
        # A rank that FAILS must not enter a barrier: its peers are inside an all-reduce / reduce-scatter, not a barrier, and
        # the mismatched collective would hold this rank (and its traceback) until the RCCL timeout.  Tear the group down
        # without synchronising and leave with the exception: the non-zero exit makes the launcher (launch_ranks /
        # torch.distributed.run) stop the other ranks.
        if dp:
            # the abort goes through private torch entry points whose blocking behaviour differs between versions: give it
            # five seconds on a thread of its own, then leave the hard way with the traceback already printed
            import threading
            import traceback
            th = threading.Thread(target=_abort_process_group, daemon=True)
            th.start()
            th.join(5.0)
            if th.is_alive():
                traceback.print_exc()
                sys.stderr.flush()
                os._exit(1)
        raise
    if dp:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.barrier()
            dist.destroy_process_group()
    return hist


if __name__ == "__main__":
    main()
