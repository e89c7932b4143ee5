"""Do the chunk borders show in a converted mel?  The seam figure of DESIGN.md §4.12, measured.

    python scripts/convert_seams.py [--log_dir RUN] [--utts 6] [--seed 0] --json convert_seams.json      (on the GPU)
    python scripts/convert_seams.py --from-json convert_seams.json --write-docs                          (anywhere)

The figure: the mean absolute frame-to-frame jump of the converted mel, mean_c |M[c, t] - M[c, t - 1]|, over the frames at
the old chunk borders t = k T, divided by the same mean over all other frames (both pooled over the utterances, frames
below the utterance's length only).  1 means the borders cannot be told from the rest.  Compared on the same utterances
and the same weights: `convert_mel` (the reference's disjoint chunks, one target utterance) and the overlapped path
(convert.Converter) at hop = T / 2 and T / 4, which takes its style from the same target utterance.

Weights: the last checkpoint of --log_dir when given, otherwise a seeded random-initialised model in eval mode (named as
such in the output: it says how the ARCHITECTURE treats a border, not what a trained model does).  Utterances: synthetic
smooth mels (slow sinusoids over time and channel), so that the jumps measured are the model's and not the input's.
One process; every step runs only when the one before it returned, under one time limit (--time-limit seconds, exit 124).
--write-docs puts the figures of a recorded run between the `convert_seams` markers of README.md."""
import argparse
import json
import os
import re
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BEGIN, END = "<!-- convert_seams:begin -->", "<!-- convert_seams:end -->"


def smooth_mel(rs, length, n_mel=80):
    import numpy as np
    t = np.arange(length)[None, :] / 100.0
    c = np.arange(n_mel)[:, None] / n_mel
    m = 0.5 + sum(a * np.sin(2 * np.pi * (f * t + g * c) + p) for a, f, g, p in
                  zip(rs.uniform(0.05, 0.15, 5), rs.uniform(0.2, 2.0, 5), rs.uniform(0.5, 3.0, 5), rs.uniform(0, 6.28, 5)))
    return np.clip(m, 0.0, 1.0).astype(np.float32)


def seam_figure(mels, T):
    """-> (mean jump at t = k T, mean jump elsewhere, their ratio, border frames, other frames)"""
    import numpy as np
    at, off = [], []
    for m in mels:
        jump = np.abs(np.diff(np.asarray(m, np.float64), axis=1)).mean(0)       # jump[t - 1] = frame t against t - 1
        t = np.arange(1, m.shape[1])
        border = t % T == 0
        at.append(jump[border])
        off.append(jump[~border])
    at, off = np.concatenate(at), np.concatenate(off)
    return float(at.mean()), float(off.mean()), float(at.mean() / off.mean()), int(at.size), int(off.size)


def measure(args):
    import numpy as np
    import torch
    import dvae_amd
    from dvae_amd import convert
    if not torch.cuda.is_available():
        raise SystemExit("convert_seams: no GPU; the conversion runs on the device or not at all")
    signal.signal(signal.SIGALRM, lambda *_: os._exit(124))
    signal.alarm(int(args.time_limit))
    dev = torch.device("cuda", torch.cuda.current_device())
    T = 64
    if args.log_dir:
        vsc, ckpt = convert.load_run(args.log_dir, dev)
        T = int(vsc.model.n_frames)
        weights = f"the last checkpoint of a trained run ({ckpt})"
    else:
        torch.manual_seed(args.seed)
        vsc = dvae_amd.ConvolutionalMulVAE("VCTK", T, 80, 32, 1e-4, 0.01, 500, False, batch_size=4, speaker_size=4, device=dev,
                                           latent_dim=32, mse_cof=10, kl_cof=10)
        weights = f"a seeded random-initialised model (torch.manual_seed({args.seed}), no training)"
    rs = np.random.RandomState(args.seed)
    lengths = [int(n) for n in rs.randint(5 * T, 8 * T, size=args.utts)]
    sources = [smooth_mel(rs, n) for n in lengths]
    target = smooth_mel(rs, 6 * T + 17)
    res = {"chunks": seam_figure([vsc.convert_mel(s, target)["converted"][:, :s.shape[1]].cpu().numpy() for s in sources], T)}
    torch.cuda.synchronize()
    for hop in (T // 2, T // 4):
        conv = convert.Converter(vsc, hop=hop, batch=args.batch)
        out = conv.convert(sources, target)
        torch.cuda.synchronize()
        assert all(tuple(o["converted"].shape) == (80, n) for o, n in zip(out, lengths))
        res[f"hop{hop}"] = seam_figure([o["converted"].cpu().numpy() for o in out], T)
    res["input"] = seam_figure(sources, T)
    vsc._check_device_errors()
    signal.alarm(0)
    keys = ("at_borders", "elsewhere", "ratio", "border_frames", "other_frames")
    return {"device": torch.cuda.get_device_name(dev), "weights": weights, "T": T, "utterances": len(sources),
            "frames": int(sum(lengths)), "seed": args.seed, "batch": args.batch,
            **{k: dict(zip(keys, v)) for k, v in res.items()}}


def sentence(r):
    T = r["T"]
    f = lambda k: f"{r[k]['ratio']:.2f} ({r[k]['at_borders']:.2e} against {r[k]['elsewhere']:.2e})"
    return (f"Measured (`scripts/convert_seams.py`, one MI355X, {r['weights']}, {r['utterances']} synthetic smooth utterances, "
            f"{r['frames']} frames, T = {T}; the mean absolute frame-to-frame jump of the converted mel at the chunk borders "
            f"t = k T over the same mean at all other frames, {r['chunks']['border_frames']} border frames): `convert_mel` "
            f"{f('chunks')}; overlapped at hop = {T // 2} {f('hop' + str(T // 2))}, at hop = {T // 4} {f('hop' + str(T // 4))}; "
            f"the inputs themselves {r['input']['ratio']:.2f}.")


def write_docs(r):
    text = BEGIN + "\n" + sentence(r) + "\n" + END
    path = os.path.join(ROOT, "README.md")
    doc = open(path).read()
    if BEGIN not in doc or END not in doc:
        raise SystemExit(f"convert_seams: README.md has no {BEGIN} ... {END} block")
    open(path, "w").write(re.sub(re.escape(BEGIN) + ".*?" + re.escape(END), lambda _: text, doc, flags=re.S))
    print("convert_seams: wrote the figures into README.md")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--log_dir", default=None, help="a trained run (config.json, checkpoints/); default: random-initialised")
    ap.add_argument("--utts", type=int, default=6)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--time-limit", type=int, default=300, help="seconds for the whole measurement (exit code 124)")
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
