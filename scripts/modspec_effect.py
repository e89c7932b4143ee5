"""What do the over-smoothing scores and the modulation-spectrum postfilter do on a known smoothing, and what do the launches
cost?  The figures of DESIGN.md §4.14, measured.

    python scripts/modspec_effect.py [--utts 6] [--seed 0] [--D 64] --json modspec_effect.json      (on the GPU)
    python scripts/modspec_effect.py --from-json modspec_effect.json --write-docs                   (anywhere)

"Natural" mels: seeded synthetic smooth random trajectories in [0, 1], --utts utterances of 300 ... 500 frames.  "Generated"
mels: the same with every bin smoothed by a 5-frame moving average — a stand-in for an over-smoothing decoder whose effect
is known.  Reported: msd_db and gv_ratio_db of generated against natural (dvae_amd.modspec.ModSpec.score), before the
postfilter and after it at alpha = 0.5 and 1 with the statistics of the two sets themselves; and the device-event time of
each launch of csrc/modspec.hip at that size and at 2048 windows (3 warm-up calls, then the minimum and median of 10).  No
trained model and no speech corpus enter: what the postfilter does to the SOUND of a real conversion is not measured here.
One process, one time limit (--time-limit seconds, exit 124).  --write-docs puts the figures of a recorded run between the
`modspec_effect` markers of README.md."""
import argparse
import json
import os
import re
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BEGIN, END = "<!-- modspec_effect:begin -->", "<!-- modspec_effect:end -->"


def natural_mel(rs, length, n_mel=80):
    """a smooth random trajectory per bin: a 9-frame moving average of uniform noise, stretched, plus a little white noise"""
    import numpy as np
    noise = rs.rand(n_mel, length + 8)
    slow = np.stack([noise[:, j:j + length] for j in range(9)]).mean(0)
    return np.clip(0.5 + 2.5 * (slow - 0.5) + 0.05 * (rs.rand(n_mel, length) - 0.5), 0.0, 1.0).astype(np.float32)


def smoothed(mel, width=5):
    """every bin's `width`-frame moving average (edges: the frames there are)"""
    import numpy as np
    m = np.asarray(mel, np.float64)
    pad = np.pad(m, ((0, 0), (width // 2, width // 2)), mode="edge")
    return np.stack([pad[:, j:j + m.shape[1]] for j in range(width)]).mean(0).astype(np.float32)


def timed(fn, warmup=3, calls=10):
    import numpy as np
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(min_us=1e3 * float(np.min(ms)), median_us=1e3 * float(np.median(ms)))


def launch_times(ms, modspec, convert, mels, up):
    """each launch of csrc/modspec.hip alone on the windows of `mels`"""
    import numpy as np
    import torch
    p, packed = ms.pack(mels)
    windows = convert.mel_to_windows(packed, p["utt_d"], p["win_d"], ms.D)
    n, C = windows.shape[0], windows.shape[1]
    rows = modspec.modspec_windows(windows, ms.tw)
    order, first = up(np.arange(n), np.int32), up(np.asarray([0, n // 2, n]), np.int32)
    st = ms.stats({"all": mels})
    stat = [torch.from_numpy(a).to(ms.device) for a in (st.mean("all"), st.std("all"), st.mean("all") - 0.5, st.std("all"))]
    return dict(windows=int(n), utterances=len(mels),
                mel_gv=timed(lambda: modspec.mel_gv(packed, p["utt_d"])),
                modspec_windows=timed(lambda: modspec.modspec_windows(windows, ms.tw)),
                modspec_group_sum=timed(lambda: modspec.modspec_group_sum(rows, order, first, n, C, ms.D)),
                modspec_filter=timed(lambda: modspec.modspec_filter(windows, ms.tw, *stat, 1.0, 12.0)))


def measure(args):
    import numpy as np
    import torch
    import dvae_amd  # noqa: F401
    from dvae_amd import convert, modspec
    from dvae_amd.packed import upload
    if not torch.cuda.is_available():
        raise SystemExit("modspec_effect: no GPU; the instruments run on the device or not at all")
    signal.signal(signal.SIGALRM, lambda *_: os._exit(124))
    signal.alarm(int(args.time_limit))
    dev = torch.device("cuda", torch.cuda.current_device())
    ms = modspec.ModSpec(dev, args.D)
    rs = np.random.RandomState(args.seed)
    lengths = [int(n) for n in rs.randint(300, 501, size=args.utts)]
    natural = [natural_mel(rs, n) for n in lengths]
    generated = [smoothed(m) for m in natural]
    sn, sg = ms.stats({"natural": natural}), ms.stats({"generated": generated})
    pick = lambda sc: dict(msd_db=sc["msd_db"], gv_ratio_db=sc["gv_ratio_db"])
    res = {"before": pick(ms.score(sg, "generated", sn, "natural"))}
    for alpha in (0.5, 1.0):
        out = ms.postfilter(generated, (sn, "natural"), (sg, "generated"), alpha=alpha, max_gain_db=args.max_gain_db)
        assert all(tuple(o.shape) == (80, n) for o, n in zip(out, lengths))
        res[f"alpha{alpha}"] = pick(ms.score(ms.stats({"filtered": out}), "filtered", sn, "natural"))
    up = lambda a, dt: upload(a, dev, dt)
    res["times"] = launch_times(ms, modspec, convert, natural, up)
    per = int(res["times"]["windows"] // len(natural)) + 1
    big = [natural_mel(rs, ms.hop * (per - 1) + ms.D) for _ in range(-(-2048 // per))]
    big_n = sum(len(convert.window_plan(m.shape[1], ms.D, ms.hop)) for m in big)
    while big_n > 2048:                                    # exactly 2048 windows: shorten the last utterance
        big[-1] = big[-1][:, :big[-1].shape[1] - ms.hop]
        big_n -= 1
    res["times_2048"] = launch_times(ms, modspec, convert, big, up)
    torch.cuda.synchronize()
    signal.alarm(0)
    return {"device": torch.cuda.get_device_name(dev), "D": ms.D, "hop": ms.hop, "utterances": len(natural),
            "frames": int(sum(lengths)), "seed": args.seed, "max_gain_db": args.max_gain_db, **res}


def sentence(r):
    f = lambda k: f"msd {r[k]['msd_db']:.2f} dB, gv ratio {r[k]['gv_ratio_db']:+.2f} dB"
    t = lambda blk: ", ".join(f"`dvae_{k}` {r[blk][k]['min_us']:.0f} / {r[blk][k]['median_us']:.0f}"
                              for k in ("mel_gv", "modspec_windows", "modspec_group_sum", "modspec_filter"))
    return (f"Measured (`scripts/modspec_effect.py`, one MI355X, {r['utterances']} seeded synthetic smooth utterances, {r['frames']} "
            f"frames, \"generated\" = a 5-frame moving average of every bin, D = {r['D']}, hop = {r['hop']}, max gain "
            f"{r['max_gain_db']:g} dB; no trained model, no speech): generated against natural {f('before')}; after the postfilter at "
            f"alpha = 0.5 {f('alpha0.5')}; at alpha = 1 {f('alpha1.0')}.  Device-event time per launch, minimum / median of 10 in "
            f"µs: at {r['times']['windows']} windows {t('times')}; at {r['times_2048']['windows']} windows {t('times_2048')}.  The "
            f"times are recorded, not judged: there is no earlier version to compare with.")


def write_docs(r):
    text = BEGIN + "\n" + sentence(r) + "\n" + END
    path = os.path.join(ROOT, "README.md")
    doc = open(path).read()
    if BEGIN not in doc or END not in doc:
        raise SystemExit(f"modspec_effect: README.md has no {BEGIN} ... {END} block")
    open(path, "w").write(re.sub(re.escape(BEGIN) + ".*?" + re.escape(END), lambda _: text, doc, flags=re.S))
    print("modspec_effect: wrote the figures into README.md")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--utts", type=int, default=6)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--D", type=int, default=64, help="frames per window (even, 8 ... 128)")
    ap.add_argument("--max-gain-db", type=float, default=12.0)
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
