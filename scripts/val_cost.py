"""What a validation batch (VariationalBaseModelVAE.validate) costs beside a training step, measured.

    python scripts/val_cost.py [--batch 64] [--frames 128] [--rounds 6] [--steps 20] --json val_cost.json      (on the GPU)
    python scripts/val_cost.py --from-json val_cost.json --write-docs                                          (anywhere)

One trainer of the flagship workload (B = 64 / T = 128, the default arithmetic) in ONE process.  After a warm-up, blocks of
`--steps` replayed training steps alternate with blocks of `--steps` validation batches (the eval-mode forward on a private
style noise, dvae_pair_metrics, dvae_group_sum_f64 — eager launches, as `validate` issues them), each block timed with a host
clock around a device synchronise, so that whatever else the host and the device are doing falls on both alike.  Reported:
the median block of either, the spread, their ratio, and — with device events — the two new launches alone.  Nothing is
gated: the expectation from the launch list is a validation batch well under half a training step (it is forward only).
--write-docs puts the figures of a recorded run between the `val_cost` markers of README.md."""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BEGIN, END = "<!-- val_cost:begin -->", "<!-- val_cost:end -->"


def measure(args):
    import torch
    import dvae_amd
    from dvae_amd import ops
    from dvae_amd.data import SyntheticPairs
    if not torch.cuda.is_available():
        raise SystemExit("val_cost: no GPU; a time is measured on the device or not at all")
    dev = torch.device("cuda", torch.cuda.current_device())
    ops.set_compute_dtype(args.dtype)
    B, T, G = args.batch, args.frames, 10
    x1, x2, spk = SyntheticPairs(B, T, n_speakers=G, seed=1234, device=dev).batch()
    spk32 = spk.to(torch.int32).contiguous()
    torch.manual_seed(1234)
    w = dvae_amd.ConvolutionalMulVAE("VCTK", T, 80, 32, 1e-4, 0.01, 500, False, batch_size=B, speaker_size=4, device=dev,
                                     latent_dim=32, mse_cof=10, kl_cof=10)
    w.model.train()
    w.enable_graph(True)
    for _ in range(args.warmup):              # the first step is eager, the second captures, the rest replay
        w.step(x1, x2, spk, train=True)
    assert w._graph is not None
    m = w.model
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    sums = torch.zeros((G + 1, 8), dtype=torch.float64, device=dev)
    counts, bad = torch.zeros(G + 1, dtype=torch.int64, device=dev), torch.zeros(G + 1, dtype=torch.int64, device=dev)

    def val_batch():
        eps = torch.randn((B, m.speaker_size), device=dev, generator=gen)
        outs = m.forward_full(x1, x2, train=False, eps_style=eps)
        rows = ops.pair_metrics(x1, x2, *outs, w.mse_cof, w.kl_cof)
        ops.group_sum(rows, spk32, sums, counts, bad)
        return outs, rows

    def block(kind):
        if kind == "val":
            m.eval()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "val":
            with torch.no_grad():
                for _ in range(args.steps):
                    val_batch()
        else:
            for _ in range(args.steps):
                w.step_async(x1, x2, spk)
        torch.cuda.synchronize()
        dt = 1e3 * (time.perf_counter() - t0) / args.steps
        m.train()
        return dt

    block("val")                               # warm-up of the eval-mode path
    times = {"train": [], "val": []}
    for _ in range(args.rounds):
        for kind in ("train", "val"):
            times[kind].append(block(kind))
    ops.lstm_pers_check()

    # the two new launches alone, on the outputs of one validation forward
    m.eval()
    with torch.no_grad():
        outs, rows = val_batch()
    m.train()
    out = torch.empty_like(rows)

    def added():
        ops.pair_metrics(x1, x2, *outs, w.mse_cof, w.kl_cof, out=out)
        ops.group_sum(out, spk32, sums, counts, bad)

    for _ in range(5):
        added()
    reps = 50
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        added()
    b.record()
    torch.cuda.synchronize()

    def summary(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "blocks_ms": v}

    tr, va = summary(times["train"]), summary(times["val"])
    return {"device": torch.cuda.get_device_name(dev), "batch": B, "frames": T, "dtype": args.dtype, "rounds": args.rounds,
            "steps_per_block": args.steps, "warmup_steps": args.warmup, "train_step": tr, "val_batch": va,
            "ratio": va["median_ms"] / tr["median_ms"], "launches_alone_ms": a.elapsed_time(b) / reps,
            "pairs_counted": int(counts[G].item())}


def sentence(r):
    tr, va = r["train_step"], r["val_batch"]
    verdict = ("under half a training step, as the launch list suggested" if r["ratio"] < 0.5 else
               "NOT under half a training step, which the launch list had suggested")
    return (f"Measured (`scripts/val_cost.py`, one MI355X, one process, B = {r['batch']} / T = {r['frames']}, {r['dtype']}, "
            f"{r['rounds']} alternating blocks of {r['steps_per_block']} each): {tr['median_ms']:.3f} ms per replayed training "
            f"step ({tr['min_ms']:.3f} .. {tr['max_ms']:.3f}), {va['median_ms']:.3f} ms per validation batch "
            f"({va['min_ms']:.3f} .. {va['max_ms']:.3f}; eager launches): {r['ratio']:.2f} of a step — {verdict}.  "
            f"The two new launches alone (per-pair terms + per-speaker float64 sums), timed with device events: "
            f"{1e3 * r['launches_alone_ms']:.1f} us.")


def write_docs(r):
    text = BEGIN + "\n" + sentence(r) + "\n" + END
    path = os.path.join(ROOT, "README.md")
    doc = open(path).read()
    if BEGIN not in doc or END not in doc:
        raise SystemExit(f"val_cost: README.md has no {BEGIN} ... {END} block")
    open(path, "w").write(re.sub(re.escape(BEGIN) + ".*?" + re.escape(END), lambda _: text, doc, flags=re.S))
    print("val_cost: wrote the figures into README.md")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--dtype", default="fp32x3")
    ap.add_argument("--rounds", type=int, default=6, help="alternating blocks per kind")
    ap.add_argument("--steps", type=int, default=20, help="training steps / validation batches per block")
    ap.add_argument("--warmup", type=int, default=5)
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
