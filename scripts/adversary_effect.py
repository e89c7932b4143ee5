"""What the speaker adversary (ConvolutionalMulVAE.set_speaker_adversary) does to speaker leakage, on a
SYNTHETIC corpus, measured three ways.

    python scripts/adversary_effect.py [--speakers 6] [--utts 20] [--epochs 60] --out DIR --json adversary_effect.json   (on the GPU)
    python scripts/adversary_effect.py --from-json adversary_effect.json --write-docs                                     (anywhere)

The corpus is seeded noise: every utterance is U[0, 0.5) per mel bin and frame plus 0.4 times a fixed per-speaker mel profile
(80 numbers in [0, 1) per speaker, drawn once from the same seed), so the speaker is plainly readable from any frame and
there is no linguistic content at all.  Two runs of `python -m dvae_amd.train` from the same seed on it, one with
`--adv-weight 0` (the classifier learns, the model is untouched) and one with `--adv-weight 0.5`; then on each run
`python -m dvae_amd.probe` and `python -m dvae_amd.latents`.  Reported for both: the last epoch's `Adv/Accuracy` (the
adversary's own accuracy on the training batches), `probe`'s held-out accuracy on the content block, and `latents`' speaker
information of the content block in nats beside the speakers' entropy.  Every process is a fresh child with a time limit.
The figures are recorded, not judged; real speech is not measured.  --write-docs puts a recorded run between the
`adversary_effect` markers of README.md."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BEGIN, END = "<!-- adversary_effect:begin -->", "<!-- adversary_effect:end -->"
WEIGHTS = (0.0, 0.5)


def write_corpus(root, speakers, utts, length, seed):
    import numpy as np
    rs = np.random.RandomState(seed)
    profiles = rs.uniform(0.0, 1.0, size=(speakers, 80))
    for s in range(speakers):
        d = os.path.join(root, f"spk{s:03d}")
        os.makedirs(d, exist_ok=True)
        for u in range(utts):
            mel = rs.uniform(0.0, 0.5, size=(80, length)) + 0.4 * profiles[s][:, None]
            np.save(os.path.join(d, f"utt{u:03d}_mel.npy"), mel)
    return root


def child(module, argv, limit):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    call = "t.main(sys.argv[1:])" if module == "train" else "sys.exit(t.main(sys.argv[1:]))"      # train.main returns its history
    code = f"import dvae_amd.{module} as t, sys; {call}"
    r = subprocess.run([sys.executable, "-c", code] + [str(a) for a in argv], env=env, capture_output=True, text=True,
                       timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"adversary_effect: python -m dvae_amd.{module} failed ({r.returncode}):\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
    return r


def measure(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("adversary_effect: no GPU; the runs train on the device or not at all")
    out = os.path.abspath(args.out)
    corpus = write_corpus(os.path.join(out, "corpus"), args.speakers, args.utts, args.length, args.seed)
    runs = {}
    for w in WEIGHTS:
        log = os.path.join(out, f"weight_{w}")
        child("train", ["--train", "true", f"--dataset_fp={corpus}", f"--batch-size={args.batch}", "--latent-size=32",
                        "--speaker_size=4", f"--lr={args.lr}", f"--epochs={args.epochs}", f"--report-interval={args.epochs}",
                        "--mse_cof=10", "--kl_cof=10", f"--seed={args.seed}", "--gpu-loader=1", "--do-not-resume",
                        f"--log_dir={log}", "--adv-weight", w, "--adv-warmup-steps", args.warmup_steps if w > 0 else 0],
              args.limit)
        recs = [json.loads(line) for line in open(os.path.join(log, "logs", "DisentangledVAE_VCTK", "scalars.jsonl"))]
        child("probe", [corpus, "--log_dir", log, "--seed", args.seed], args.limit)
        child("latents", [corpus, "--log_dir", log, "--seed", args.seed], args.limit)
        probe = json.load(open(os.path.join(log, "probe.json")))
        lat = json.load(open(os.path.join(log, "latents.json")))
        runs[str(w)] = {
            "adv_accuracy": recs[-1]["Adv/Accuracy"], "adv_ce": recs[-1]["Adv/CE"], "adv_weight": recs[-1]["Adv/Weight"],
            "adv_accuracy_first_epoch": recs[0]["Adv/Accuracy"], "epochs": len(recs),
            "reconstruction_loss1": recs[-1]["Loss/Reconstruction Loss1"], "kl_z1": recs[-1]["Loss/Z1 KL Loss"],
            "probe_content_held_out_accuracy": probe["probes"]["content"]["held_out_accuracy"],
            "probe_style_held_out_accuracy": probe["probes"]["style"]["held_out_accuracy"],
            "probe_chance": probe["chance"], "held_out_chunks": probe["n_held_out_chunks"],
            "speaker_info_content": lat["speaker_info"]["content"], "speaker_info_style": lat["speaker_info"]["style"],
            "speaker_entropy": lat["speaker_entropy"], "chunks": lat["n_chunks"]}
    return {"device": torch.cuda.get_device_name(0), "speakers": args.speakers, "utts": args.utts, "length": args.length,
            "seed": args.seed, "batch": args.batch, "epochs": args.epochs, "lr": args.lr, "warmup_steps": args.warmup_steps,
            "runs": runs}


def reading(a, b):
    """what the two runs' figures say, in plain words, whichever way they came out"""
    acc = "lower" if b["adv_accuracy"] < a["adv_accuracy"] else "NOT lower"
    info = "lower" if b["speaker_info_content"] < a["speaker_info_content"] else "NOT lower"
    probe = "lower" if b["probe_content_held_out_accuracy"] < a["probe_content_held_out_accuracy"] else "NOT lower"
    return (f"With the weight on, the adversary's own accuracy is {acc}, `probe`'s content accuracy is {probe} and `latents`' "
            f"speaker information of the content block is {info} than in the monitor-only run.  On this corpus the speaker "
            "is a constant offset of every frame, and the reconstruction term (`mse_cof` times an L1 sum over the mel) sends the "
            "encoder a gradient orders of magnitude above the reversed one at this weight: one pair of runs from one seed shows "
            "how the two runs differ, not that the weight caused it.")


def sentence(r):
    a, b = r["runs"]["0.0"], r["runs"]["0.5"]
    one = lambda x: (f"`Adv/Accuracy` {x['adv_accuracy']:.3f} in the last epoch ({x['adv_accuracy_first_epoch']:.3f} in the first), "
                     f"`probe` held-out content accuracy {x['probe_content_held_out_accuracy']:.3f} (style "
                     f"{x['probe_style_held_out_accuracy']:.3f}), `latents` speaker information of the content block "
                     f"{x['speaker_info_content']:.3f} nats (style {x['speaker_info_style']:.3f}), reconstruction loss "
                     f"{x['reconstruction_loss1']:.1f}")
    return (f"Measured (`scripts/adversary_effect.py`, one MI355X) on a SYNTHETIC corpus — {r['speakers']} speakers x {r['utts']} "
            f"utterances of {r['length']} frames of seeded noise plus a fixed per-speaker mel profile, no speech in it — two runs "
            f"from seed {r['seed']}, {r['epochs']} epochs at batch {r['batch']}, lr {r['lr']} (chance {a['probe_chance']:.3f}, "
            f"speaker entropy {a['speaker_entropy']:.3f} nats, {a['held_out_chunks']} held-out chunks).  Weight 0: {one(a)}.  "
            f"Weight 0.5 (rising over the first {r['warmup_steps']} steps): {one(b)}.  {reading(a, b)}  The figures are "
            "recorded, not judged; the effect on real speech is **not measured**.")


def write_docs(r):
    text = BEGIN + "\n" + sentence(r) + "\n" + END
    path = os.path.join(ROOT, "README.md")
    doc = open(path).read()
    if BEGIN not in doc or END not in doc:
        raise SystemExit(f"adversary_effect: README.md has no {BEGIN} ... {END} block")
    doc = re.sub(re.escape(BEGIN) + ".*?" + re.escape(END), lambda _: text, doc, flags=re.S)
    open(path, "w").write(doc)
    print("adversary_effect: wrote the figures into README.md")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--speakers", type=int, default=6)
    ap.add_argument("--utts", type=int, default=20, help="utterances per speaker (probe holds every fifth out)")
    ap.add_argument("--length", type=int, default=128, help="frames per utterance (two chunks of 64)")
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=60)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--warmup-steps", type=int, default=50, help="--adv-warmup-steps of the run with weight 0.5")
    ap.add_argument("--limit", type=int, default=300, help="time limit of every child process, seconds")
    ap.add_argument("--out", default="adversary_effect_runs", help="where the corpus and the two runs go")
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
