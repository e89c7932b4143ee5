"""What the factor penalty (ConvolutionalMulVAE.set_factor_penalty) does to the figures it acts on, on a
SYNTHETIC corpus.

    python scripts/factor_effect.py [--speakers 6] [--utts 20] [--epochs 30] --out DIR --json factor_effect.json   (on the GPU)
    python scripts/factor_effect.py --from-json factor_effect.json --write-docs                                     (anywhere)

The corpus is scripts/adversary_effect.py's: seeded noise plus a fixed per-speaker mel profile, no speech in it.  Two runs of
`python -m dvae_amd.train` from the same seed on it, one with `--tc-weight 0` (the statistics are computed, the model is
untouched) and one with `--tc-weight W --shared-weight W` rising over the first steps; then on each run
`python -m dvae_amd.latents`.  Reported for both: the corpus-level total correlation of the style block, the content block
and the whole latent, the information the two blocks share, the speaker information of both blocks, the last epoch's
minibatch statistics (`Factor/...`) and the reconstruction loss.  Every process is a fresh child with a time limit.  The
figures are recorded, not judged; real speech is not measured.  --write-docs puts a recorded run between the `factor_effect`
markers of README.md."""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from adversary_effect import child, write_corpus  # noqa: E402

BEGIN, END = "<!-- factor_effect:begin -->", "<!-- factor_effect:end -->"


def measure(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("factor_effect: no GPU; the runs train on the device or not at all")
    out = os.path.abspath(args.out)
    corpus = write_corpus(os.path.join(out, "corpus"), args.speakers, args.utts, args.length, args.seed)
    runs = {}
    for name, w in (("off", 0.0), ("on", args.weight)):
        log = os.path.join(out, f"weight_{name}")
        flags = ["--tc-weight", w] + (["--shared-weight", w, "--factor-warmup-steps", args.warmup_steps] if w > 0 else [])
        child("train", ["--train", "true", f"--dataset_fp={corpus}", f"--batch-size={args.batch}", "--latent-size=32",
                        "--speaker_size=4", f"--lr={args.lr}", f"--epochs={args.epochs}", f"--report-interval={args.epochs}",
                        "--mse_cof=10", "--kl_cof=10", f"--seed={args.seed}", "--gpu-loader=1", "--do-not-resume",
                        f"--log_dir={log}"] + flags, args.limit)
        recs = [json.loads(line) for line in open(os.path.join(log, "logs", "DisentangledVAE_VCTK", "scalars.jsonl"))]
        child("latents", [corpus, "--log_dir", log, "--seed", args.seed], args.limit)
        lat = json.load(open(os.path.join(log, "latents.json")))
        last = recs[-1]
        runs[name] = {
            "tc_style": lat["blocks"]["style"]["tc"], "tc_content": lat["blocks"]["content"]["tc"],
            "tc_joint": lat["blocks"]["joint"]["tc"], "shared": lat["shared"],
            "speaker_info_style": lat["speaker_info"]["style"], "speaker_info_content": lat["speaker_info"]["content"],
            "speaker_entropy": lat["speaker_entropy"], "chunks": lat["n_chunks"], "ln_n": lat["ln_n"],
            "reconstruction_loss1": last["Loss/Reconstruction Loss1"], "kl_z1": last["Loss/Z1 KL Loss"],
            "step": {k: last[k] for k in last if k.startswith("Factor/")}, "epochs": len(recs)}
    return {"device": torch.cuda.get_device_name(0), "speakers": args.speakers, "utts": args.utts, "length": args.length,
            "seed": args.seed, "batch": args.batch, "epochs": args.epochs, "lr": args.lr, "weight": args.weight,
            "warmup_steps": args.warmup_steps, "runs": runs}


def sentence(r):
    a, b = r["runs"]["off"], r["runs"]["on"]
    one = lambda x: (f"corpus-level (`latents`, {x['chunks']} chunks, ln N = {x['ln_n']:.3f}) tc style {x['tc_style']:.3f}, content "
                     f"{x['tc_content']:.3f}, joint {x['tc_joint']:.3f}, shared {x['shared']:.3f} nats, speaker information style "
                     f"{x['speaker_info_style']:.3f} / content {x['speaker_info_content']:.3f} of {x['speaker_entropy']:.3f} nats; "
                     f"last epoch's minibatch means `Factor/TC style` {x['step']['Factor/TC style']:.3f}, `Factor/TC content` "
                     f"{x['step']['Factor/TC content']:.3f}, `Factor/Shared` {x['step']['Factor/Shared']:.3f}, `Factor/MI` "
                     f"{x['step']['Factor/MI']:.3f}; reconstruction loss {x['reconstruction_loss1']:.1f}, `Loss/Z1 KL Loss` {x['kl_z1']:.1f}")
    cmp_ = lambda k: "lower" if b[k] < a[k] else "NOT lower"
    return (f"Measured (`scripts/factor_effect.py`, one MI355X) on a SYNTHETIC corpus — {r['speakers']} speakers x {r['utts']} "
            f"utterances of {r['length']} frames of seeded noise plus a fixed per-speaker mel profile, no speech in it — two runs "
            f"from seed {r['seed']}, {r['epochs']} epochs at batch {r['batch']} (N = {2 * r['batch']} rows a step), lr {r['lr']}.  "
            f"Weights 0 (monitor): {one(a)}.  Weights {r['weight']} / {r['weight']} (rising over the first {r['warmup_steps']} "
            f"steps): {one(b)}.  With the weights on, the corpus-level joint total correlation is {cmp_('tc_joint')} and the "
            f"shared information is {cmp_('shared')} than in the monitor-only run.  An estimate on N rows cannot "
            "exceed a multiple of ln N, so the minibatch figures of a small batch are not the corpus-level ones, and the run "
            "with the weights on also ended with a different KL term: the two runs differ in more than the penalised figures.  "
            "One pair of runs from one seed shows how the two "
            "runs differ, not that the weights caused it.  The figures are recorded, not judged; the effect on real speech is "
            "**not measured**.")


def write_docs(r):
    text = BEGIN + "\n" + sentence(r) + "\n" + END
    path = os.path.join(ROOT, "README.md")
    doc = open(path).read()
    if BEGIN not in doc or END not in doc:
        raise SystemExit(f"factor_effect: README.md has no {BEGIN} ... {END} block")
    doc = re.sub(re.escape(BEGIN) + ".*?" + re.escape(END), lambda _: text, doc, flags=re.S)
    open(path, "w").write(doc)
    print("factor_effect: wrote the figures into README.md")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--speakers", type=int, default=6)
    ap.add_argument("--utts", type=int, default=20)
    ap.add_argument("--length", type=int, default=128, help="frames per utterance (two chunks of 64)")
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--weight", type=float, default=4.0, help="--tc-weight and --shared-weight of the second run")
    ap.add_argument("--warmup-steps", type=int, default=50, help="--factor-warmup-steps of the second run")
    ap.add_argument("--limit", type=int, default=300, help="time limit of every child process, seconds")
    ap.add_argument("--out", default="factor_effect_runs", help="where the corpus and the two runs go")
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
