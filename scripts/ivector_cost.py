"""What the i-vector kernels (dvae_amd.ivector) cost, measured.

    python scripts/ivector_cost.py --json ivector_cost.json                          (on the GPU)
    python scripts/ivector_cost.py --from-json ivector_cost.json --write-docs        (anywhere)

One process, nothing else on the card.  The three kernels at (U, K, D, R) = (4096, 64, 23, 32) and (4096, 256, 23, 64) on
random statistics (dvae_gmm_utt_stats on U segments of `--frames` frames each): 3 warm-up launches, then 10 launches timed
one by one between device events; the minimum and the median are reported.  Then a whole 10-iteration train_extractor at
the first shape, by the host's clock around a call that ends with the last download.  The times are recorded, not judged:
there is no earlier version to compare with.
--write-docs puts the figures of a recorded run between the `ivector_cost` markers of README.md."""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BEGIN, END = "<!-- ivector_cost:begin -->", "<!-- ivector_cost:end -->"
SHAPES = [(4096, 64, 23, 32), (4096, 256, 23, 64)]
WARMUP, REPS = 3, 10


def timed(fn):
    """-> (minimum, median) device time in milliseconds of REPS launches timed one by one after WARMUP launches"""
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return min(ts), statistics.median(ts)


def shape_inputs(dev, U, K, D, R, frames, seed=0):
    import numpy as np
    import torch
    from dvae_amd import ivector, verify
    rs = np.random.RandomState(seed)
    ubm = verify.DiagGMM(np.full(K, 1.0 / K), rs.randn(K, D) * 2.0, rs.uniform(0.5, 1.5, (K, D)))
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    feats = (torch.randn((U * frames, D + 1), device=dev, generator=g) * 2.0).contiguous()
    segs = np.stack([np.arange(U, dtype=np.int64) * frames, np.full(U, frames, np.int64)], axis=1)
    T = ivector.initial_T(K, D, R, seed)
    return ubm, feats, segs, T


def measure(args):
    import numpy as np
    import torch
    from dvae_amd import ivector
    from dvae_amd._lib import check, ptr, stream
    from dvae_amd.packed import upload
    if not torch.cuda.is_available():
        raise SystemExit("ivector_cost: no GPU; a time is measured on the device or not at all")
    dev = torch.device("cuda", torch.cuda.current_device())
    L = ivector._lib()
    out = {"device": torch.cuda.get_device_name(dev), "frames": args.frames, "warmup": WARMUP, "reps": REPS, "shapes": []}
    keep = None
    for U, K, D, R in SHAPES:
        ubm, feats, segs, T = shape_inputs(dev, U, K, D, R, args.frames)
        a, mu, prec = (upload(t, dev) for t in ubm.tables())
        sg = upload(segs, dev, np.int64)
        n = torch.empty((U, K), device=dev, dtype=torch.float64)
        f = torch.empty((U, K * D), device=dev, dtype=torch.float64)
        Td, Pd = upload(T, dev, np.float64), upload(ivector.gram(T, D), dev, np.float64)
        w = torch.empty((U, R), device=dev, dtype=torch.float64)
        S = torch.empty((U, R, R), device=dev, dtype=torch.float64)
        ll = torch.empty((U,), device=dev, dtype=torch.float64)
        ws = torch.empty(int(L.dvae_ivec_ws_bytes(U, K, D, R)), device=dev, dtype=torch.uint8)
        A = torch.empty((K, R, R), device=dev, dtype=torch.float64)
        C = torch.empty((K * D, R), device=dev, dtype=torch.float64)
        Ss = torch.empty((R, R), device=dev, dtype=torch.float64)

        def stats():
            check(L.dvae_gmm_utt_stats(ptr(feats), D + 1, 1, D, ptr(sg), U, ptr(a), ptr(mu), ptr(prec), K, ptr(n), ptr(f),
                                       stream()), "utt_stats")

        def post():
            check(L.dvae_ivec_posterior(ptr(n), ptr(f), ptr(Td), ptr(Pd), U, K, D, R, ptr(w), ptr(S), ptr(ll), stream()), "posterior")

        def post_w():
            check(L.dvae_ivec_posterior(ptr(n), ptr(f), ptr(Td), ptr(Pd), U, K, D, R, ptr(w), None, None, stream()), "posterior")

        def acc():
            check(L.dvae_ivec_accumulate(ptr(n), ptr(f), ptr(w), ptr(S), U, K, D, R, ptr(ws), ptr(A), ptr(C), ptr(Ss), stream()),
                  "accumulate")

        row = {"U": U, "K": K, "D": D, "R": R, "ws_bytes": int(ws.numel())}
        for name, fn in (("utt_stats", stats), ("posterior", post), ("posterior_w_only", post_w), ("accumulate", acc)):
            lo, med = timed(fn)
            row[name + "_min_ms"], row[name + "_median_ms"] = lo, med
        out["shapes"].append(row)
        if keep is None:
            keep = (n.clone(), f.clone(), R)
        del feats, S, ws
    n, f, R = keep
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, lls = ivector.train_extractor(n, f, R, iters=10, seed=0)
    torch.cuda.synchronize()
    out["train_10_iterations_s"] = time.perf_counter() - t0
    out["train_bound_first_last"] = [lls[0], lls[-1]]
    return out


def sentence(r):
    parts = []
    for s in r["shapes"]:
        parts.append(f"at (U, K, D, R) = ({s['U']}, {s['K']}, {s['D']}, {s['R']}): `dvae_gmm_utt_stats` "
                     f"{s['utt_stats_min_ms']:.3f} / {s['utt_stats_median_ms']:.3f} ms, `dvae_ivec_posterior` with S and ll "
                     f"{s['posterior_min_ms']:.3f} / {s['posterior_median_ms']:.3f} ms (w alone "
                     f"{s['posterior_w_only_min_ms']:.3f} / {s['posterior_w_only_median_ms']:.3f} ms), `dvae_ivec_accumulate` "
                     f"{s['accumulate_min_ms']:.3f} / {s['accumulate_median_ms']:.3f} ms ({s['ws_bytes'] / 2 ** 20:.1f} MiB of "
                     f"workspace)")
    return (f"Measured (`scripts/ivector_cost.py`, one MI355X, one process, nothing else on the card; utterances of "
            f"{r['frames']} random frames; minimum / median of {r['reps']} launches timed one by one between device events "
            f"after {r['warmup']} warm-ups): " + "; ".join(parts) + f".  A whole 10-iteration `train_extractor` at the first "
            f"shape, host clock: {r['train_10_iterations_s']:.2f} s.  The times are recorded, not judged: there is no earlier "
            f"version to compare with.  No speech corpus was available: figures on real speech (cosine similarity, EER) are "
            f"**not measured**.")


def write_docs(r):
    text = BEGIN + "\n" + sentence(r) + "\n" + END
    path = os.path.join(ROOT, "README.md")
    doc = open(path).read()
    if BEGIN not in doc or END not in doc:
        raise SystemExit(f"ivector_cost: README.md has no {BEGIN} ... {END} block")
    doc = re.sub(re.escape(BEGIN) + ".*?" + re.escape(END), lambda _: text, doc, flags=re.S)
    open(path, "w").write(doc)
    print("ivector_cost: wrote the figures into README.md")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=200, help="frames per utterance of the statistics kernel's input")
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
