"""What the smoothing penalty (ConvolutionalMulVAE.set_smoothing_penalty) does to the figures it acts on, on a
SYNTHETIC corpus.

    python scripts/msloss_effect.py [--speakers 6] [--utts 20] [--epochs 30] --out DIR --json msloss_effect.json   (on the GPU)
    python scripts/msloss_effect.py --from-json msloss_effect.json --write-docs                                     (anywhere)

The corpus is scripts/adversary_effect.py's: seeded noise plus a fixed per-speaker mel profile, no speech in it; the last
`--held` utterances of every speaker are moved to a directory of their own before anything trains.  Two runs of
`python -m dvae_amd.train` from the same seed on the rest, one with `--ms-loss-weight 0` (the statistics are computed, the model
is untouched) and one with `--ms-loss-weight W --gv-loss-weight W` rising over the first steps.  Reported for both: the last
epoch's `Smooth/...` figures and reconstruction loss, `modspec.score` of the held-out reconstructions (rec_hat of an inference
pass, per 64-frame chunk) against their inputs, and on one held-out batch the ratio of the gradient norms at rec_hat, unit
penalty against the L1 term: the L1 terms are sums over 80 T elements times mse_cof and the penalty is a mean, so that ratio
says which weights make the penalty visible.  Every training run is a fresh child with a time limit.  The figures are
recorded, not judged; real speech is not measured.  --write-docs puts a recorded run between the `msloss_effect` markers of
README.md."""
import argparse
import glob
import json
import os
import re
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from adversary_effect import child, write_corpus  # noqa: E402

BEGIN, END = "<!-- msloss_effect:begin -->", "<!-- msloss_effect:end -->"
T = 64


def held_out_batches(held, batch, dev):
    """per speaker the held-out utterances cut into chunks of T frames, chunk i paired with chunk i + 1: (x1, x2) batches"""
    import numpy as np
    import torch
    a, b = [], []
    for spk in sorted(os.listdir(held)):
        chunks = []
        for f in sorted(glob.glob(os.path.join(held, spk, "*.npy"))):
            mel = np.load(f).astype(np.float32)
            chunks += [mel[:, t:t + T] for t in range(0, mel.shape[1] - T + 1, T)]
        for i in range(len(chunks)):
            a.append(chunks[i])
            b.append(chunks[(i + 1) % len(chunks)])
    x1, x2 = torch.from_numpy(np.stack(a)).to(dev), torch.from_numpy(np.stack(b)).to(dev)
    return [(x1[i:i + batch], x2[i:i + batch]) for i in range(0, len(a) - batch + 1, batch)]


def held_out_figures(log, held, args):
    """the trained model of `log` on the held-out chunks: modspec.score of rec_hat against the inputs, and the gradient norms"""
    import torch
    import dvae_amd
    from dvae_amd import modspec, ops
    dev = torch.device("cuda", torch.cuda.current_device())
    w = dvae_amd.ConvolutionalMulVAE("VCTK", T, 80, 32, args.lr, 0.01, 500, False, batch_size=args.batch, speaker_size=4,
                                     device=dev, latent_dim=32, mse_cof=10, kl_cof=10)
    w.load_last_model(os.path.join(log, "checkpoints"), logging_func=lambda *_: None)
    w.set_smoothing_penalty(None)
    batches = held_out_batches(held, args.batch, dev)
    w.model.eval()
    torch.manual_seed(args.seed)
    rec, inp = [], []
    with torch.no_grad():
        for x1, x2 in batches:
            rec_hat = w.model.forward_full(x1, x2, train=False)[1]
            rec += list(rec_hat.clamp(0.0, 1.0))
            inp += list(x1) + list(x2)
    ms = modspec.ModSpec(dev, D=T)
    st = ms.stats({"rec": rec, "in": inp})
    sc = ms.score(st, "rec", st, "in")
    # one held-out batch in training mode: the gradient of the L1-and-KL loss and of the unit penalties at rec_hat
    w.model.train()
    x1, x2 = batches[0]
    outs = w.model.forward_full(x1, x2)
    vec = w.losses_vector_full(x1, x2, *outs)
    seed = torch.zeros(8, device=dev)
    seed[0] = 1.0
    (g_loss,) = torch.autograd.grad([vec], [outs[1]], [seed])
    norms = {"loss": float(g_loss.double().norm())}
    aux = torch.zeros(5, device=dev)
    for name, pair in (("ms", (1.0, 0.0)), ("gv", (0.0, 1.0))):
        y = outs[1].detach().clone().requires_grad_(True)
        pen = ops.SmoothingPenaltyFn.apply(y, x1, x2, T, args.floor, torch.tensor(pair, device=dev), aux)
        (g,) = torch.autograd.grad([pen], [y], [ops.unit_seed(dev)])
        norms[name] = float(g.double().norm())
    return {"msd_db": sc["msd_db"], "gv_ratio_db": sc["gv_ratio_db"], "chunks": len(rec), "grad_norms_at_rec_hat": norms}


def measure(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("msloss_effect: no GPU; the runs train on the device or not at all")
    out = os.path.abspath(args.out)
    corpus, held = os.path.join(out, "corpus"), os.path.join(out, "held_out")
    write_corpus(corpus, args.speakers, args.utts + args.held, args.length, args.seed)
    for spk in sorted(os.listdir(corpus)):
        os.makedirs(os.path.join(held, spk), exist_ok=True)
        for f in sorted(glob.glob(os.path.join(corpus, spk, "*.npy")))[args.utts:]:
            shutil.move(f, os.path.join(held, spk, os.path.basename(f)))
    runs = {}
    for name, w in (("off", 0.0), ("on", args.weight)):
        log = os.path.join(out, f"weight_{name}")
        flags = ["--ms-loss-weight", w, "--ms-loss-floor", args.floor]
        if w > 0:
            flags += ["--gv-loss-weight", w, "--ms-loss-warmup-steps", args.warmup_steps]
        child("train", ["--train", "true", f"--dataset_fp={corpus}", f"--batch-size={args.batch}", "--latent-size=32",
                        "--speaker_size=4", f"--lr={args.lr}", f"--epochs={args.epochs}", f"--report-interval={args.epochs}",
                        "--mse_cof=10", "--kl_cof=10", f"--seed={args.seed}", "--gpu-loader=1", "--do-not-resume",
                        f"--log_dir={log}"] + flags, args.limit)
        recs = [json.loads(line) for line in open(os.path.join(log, "logs", "DisentangledVAE_VCTK", "scalars.jsonl"))]
        last = recs[-1]
        runs[name] = {"reconstruction_loss1_hat": last["Loss/Reconstruction Loss1 hat"],
                      "reconstruction_loss1": last["Loss/Reconstruction Loss1"], "kl_z1": last["Loss/Z1 KL Loss"],
                      "step": {k: last[k] for k in last if k.startswith("Smooth/")}, "epochs": len(recs),
                      "held_out": held_out_figures(log, held, args)}
    return {"device": torch.cuda.get_device_name(0), "speakers": args.speakers, "utts": args.utts, "held": args.held,
            "length": args.length, "seed": args.seed, "batch": args.batch, "epochs": args.epochs, "lr": args.lr,
            "weight": args.weight, "floor": args.floor, "warmup_steps": args.warmup_steps, "runs": runs}


def sentence(r):
    a, b = r["runs"]["off"], r["runs"]["on"]
    n = a["held_out"]["grad_norms_at_rec_hat"]
    one = lambda x: (f"last epoch's means `Smooth/MS distance dB` {x['step']['Smooth/MS distance dB']:.3f}, `Smooth/GV ratio dB` "
                     f"{x['step']['Smooth/GV ratio dB']:.3f}, `Smooth/MS loss` {x['step']['Smooth/MS loss']:.3f}, `Smooth/GV loss` "
                     f"{x['step']['Smooth/GV loss']:.3f}; reconstruction loss {x['reconstruction_loss1']:.1f} (hat "
                     f"{x['reconstruction_loss1_hat']:.1f}); held-out reconstructions against their inputs (`modspec.score`, "
                     f"{x['held_out']['chunks']} chunks) msd {x['held_out']['msd_db']:.3f} dB, gv ratio {x['held_out']['gv_ratio_db']:.3f} dB")
    cmp_ = lambda f: "lower" if f(b) < f(a) else "NOT lower"
    return (f"Measured (`scripts/msloss_effect.py`, one MI355X) on a SYNTHETIC corpus — {r['speakers']} speakers x {r['utts']} "
            f"utterances of {r['length']} frames of seeded noise plus a fixed per-speaker mel profile, no speech in it, and "
            f"{r['held']} more utterances a speaker held out — two runs from seed {r['seed']}, {r['epochs']} epochs at batch "
            f"{r['batch']}, lr {r['lr']}, windows of 64 frames, floor {r['floor']}.  The L1 terms are sums over 80 T elements times "
            f"`mse_cof` and the penalty is a mean: on one held-out batch of the monitor-only model the gradient at rec_hat has the "
            f"norm {n['loss']:.4g} from the loss, {n['ms']:.4g} from L_ms and {n['gv']:.4g} from L_gv at weight 1 (ratios "
            f"{n['ms'] / n['loss']:.3g} and {n['gv'] / n['loss']:.3g}), so weights of the order of {n['loss'] / max(n['ms'], 1e-30):.0f} "
            f"and {n['loss'] / max(n['gv'], 1e-30):.0f} bring the terms to the size of the loss's gradient; the second run used "
            f"{r['weight']:g} for both.  Weights 0 (monitor): {one(a)}.  Weights {r['weight']:g} / {r['weight']:g} (rising over the "
            f"first {r['warmup_steps']} steps): {one(b)}.  With the weights on, the held-out modulation-spectrum distance is "
            f"{cmp_(lambda x: x['held_out']['msd_db'])}, the held-out |gv ratio| is {cmp_(lambda x: abs(x['held_out']['gv_ratio_db']))} "
            f"and the reconstruction loss of rec_hat is {cmp_(lambda x: x['reconstruction_loss1_hat'])} than in the monitor-only run.  One pair "
            "of runs from one seed shows how the two runs differ, not that the weights caused it.  The figures are recorded, not "
            "judged; the effect on real speech is **not measured**.")


def write_docs(r):
    text = BEGIN + "\n" + sentence(r) + "\n" + END
    path = os.path.join(ROOT, "README.md")
    doc = open(path).read()
    if BEGIN not in doc or END not in doc:
        raise SystemExit(f"msloss_effect: README.md has no {BEGIN} ... {END} block")
    doc = re.sub(re.escape(BEGIN) + ".*?" + re.escape(END), lambda _: text, doc, flags=re.S)
    open(path, "w").write(doc)
    print("msloss_effect: wrote the figures into README.md")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--speakers", type=int, default=6)
    ap.add_argument("--utts", type=int, default=20)
    ap.add_argument("--held", type=int, default=4, help="held-out utterances per speaker")
    ap.add_argument("--length", type=int, default=128, help="frames per utterance (two chunks of 64)")
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--weight", type=float, default=1000.0, help="--ms-loss-weight and --gv-loss-weight of the second run")
    ap.add_argument("--floor", type=float, default=0.003, help="--ms-loss-floor of both runs")
    ap.add_argument("--warmup-steps", type=int, default=50, help="--ms-loss-warmup-steps of the second run")
    ap.add_argument("--limit", type=int, default=300, help="time limit of every child process, seconds")
    ap.add_argument("--out", default="msloss_effect_runs", help="where the corpus and the two runs go")
    ap.add_argument("--json", default=None, help="write the result here as well as to stdout")
    ap.add_argument("--from-json", default=None, help="a recorded result: nothing is measured")
    ap.add_argument("--write-docs", action="store_true", help="put the figures into README.md")
    args = ap.parse_args(argv)
    if args.from_json:
        r = json.load(open(args.from_json))
    else:
        r = measure(args)
        if args.json:
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            json.dump(r, open(args.json, "w"), indent=1)
    print(json.dumps(r))
    print(sentence(r))
    if args.write_docs:
        write_docs(r)
    return 0


if __name__ == "__main__":
    sys.exit(main())
