"""What the weight average (optim.FlatAdam.set_ema) costs per replayed step, measured.

    python scripts/ema_cost.py [--batch 64] [--frames 128] [--rounds 8] [--steps 30] --json ema_cost.json      (on the GPU)
    python scripts/ema_cost.py --from-json ema_cost.json --write-docs                                          (anywhere)

Two trainers of the flagship workload (B = 64 / T = 128, fp32x3) in ONE process, one with the average off and one with it
on, each replaying its own captured hipGraph on the same batch.  After a warm-up of both they are timed in alternating
blocks of `--steps` steps (off, on, off, on, ...; a host clock around a block that ends in a device synchronise), so that
whatever else the host and the device are doing falls on both alike.  Reported: the median block of either, the spread
(min .. max) of the blocks, the difference of the medians, and — with device events, on the trainer's own buffers — the two
added launches alone (tick + sweep) with the rate the sweep reaches over its 12 bytes per parameter.
--write-docs puts the figures of a recorded run between the `ema_cost` markers of DESIGN.md §4.10 and README.md."""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BEGIN, END = "<!-- ema_cost:begin -->", "<!-- ema_cost:end -->"


def measure(args):
    import torch
    import dvae_amd
    from dvae_amd import _lib, ops
    from dvae_amd.data import SyntheticPairs
    if not torch.cuda.is_available():
        raise SystemExit("ema_cost: no GPU; a time is measured on the device or not at all")
    dev = torch.device("cuda", torch.cuda.current_device())
    ops.set_compute_dtype(args.dtype)
    B, T = args.batch, args.frames
    x1, x2, spk = SyntheticPairs(B, T, n_speakers=10, seed=1234, device=dev).batch()

    def trainer(decay):
        torch.manual_seed(1234)
        w = dvae_amd.ConvolutionalMulVAE("VCTK", T, 80, 32, 1e-4, 0.01, 500, False, batch_size=B, speaker_size=4,
                                         device=dev, latent_dim=32, mse_cof=10, kl_cof=10)
        w.model.train()
        if decay:
            w.optimizer.set_ema(decay)
        w.enable_graph(True)
        for _ in range(args.warmup):          # the first step is eager, the second captures, the rest replay
            w.step(x1, x2, spk, train=True)
        assert w._graph is not None
        return w

    pair = {"off": trainer(0.0), "on": trainer(args.decay)}

    def block(w):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            w.step_async(x1, x2, spk)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps

    times = {"off": [], "on": []}
    for _ in range(args.rounds):
        for name in ("off", "on"):
            times[name].append(block(pair[name]))
    ops.lstm_pers_check()

    # the two added launches alone, on the buffers of the trainer that has them
    opt = pair["on"].optimizer
    L, st = _lib.lib(), _lib.stream()

    def added():
        _lib.check(L.dvae_ema_tick(opt.ema_state.data_ptr(), None, None, st), "dvae_ema_tick")
        _lib.check(L.dvae_ema_update(opt.ema.data_ptr(), opt.flat_p.data_ptr(), opt.numel, opt.ema_state.data_ptr(), st),
                   "dvae_ema_update")

    for _ in range(5):
        added()
    reps = 50
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        added()
    b.record()
    torch.cuda.synchronize()
    launches_ms = a.elapsed_time(b) / reps
    stats = opt.ema_stats()

    def summary(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "blocks_ms": v}

    off, on = summary(times["off"]), summary(times["on"])
    n = opt.numel
    return {"device": torch.cuda.get_device_name(dev), "batch": B, "frames": T, "dtype": args.dtype, "decay": args.decay,
            "rounds": args.rounds, "steps_per_block": args.steps, "warmup_steps": args.warmup, "params": n,
            "step_off": off, "step_on": on, "difference_ms": on["median_ms"] - off["median_ms"],
            "launches_alone_ms": launches_ms, "sweep_bytes": 12 * n, "sweep_GBps": 12 * n / (launches_ms * 1e-3) / 1e9,
            "expected_ms_from_arithmetic": [0.25, 0.30], "updates_counted": stats["updates"]}


def sentence(r):
    off, on = r["step_off"], r["step_on"]
    d, lo, hi = r["difference_ms"], *r["expected_ms_from_arithmetic"]
    noise = max(off["max_ms"] - off["min_ms"], on["max_ms"] - on["min_ms"])
    verdict = (f"inside the spread of the blocks ({noise:.3f} ms)" if abs(d) <= noise else
               f"against an expectation of {lo}-{hi} ms from arithmetic" + (" — more than twice that" if d > 2 * hi else ""))
    return (f"Measured (`scripts/ema_cost.py`, one MI355X, one process, B = {r['batch']} / T = {r['frames']}, {r['dtype']}, "
            f"{r['rounds']} alternating blocks of {r['steps_per_block']} replayed steps each): "
            f"{off['median_ms']:.3f} ms per step with the average off ({off['min_ms']:.3f} .. {off['max_ms']:.3f}), "
            f"{on['median_ms']:.3f} ms with it on ({on['min_ms']:.3f} .. {on['max_ms']:.3f}): a difference of {d:+.3f} ms, "
            f"{verdict}.  The two added launches alone, timed with device events over {r['params']:,} parameters: "
            f"{r['launches_alone_ms']:.3f} ms, {r['sweep_GBps']:.0f} GB/s over their 12 bytes per parameter.")


def write_docs(r):
    text = BEGIN + "\n" + sentence(r) + "\n" + END
    for name in ("DESIGN.md", "README.md"):
        path = os.path.join(ROOT, name)
        doc = open(path).read()
        if BEGIN not in doc or END not in doc:
            raise SystemExit(f"ema_cost: {name} has no {BEGIN} ... {END} block")
        doc = re.sub(re.escape(BEGIN) + ".*?" + re.escape(END), lambda _: text, doc, flags=re.S)
        open(path, "w").write(doc)
        print(f"ema_cost: wrote the figures into {name}")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--dtype", default="fp32x3")
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--rounds", type=int, default=8, help="alternating blocks per variant")
    ap.add_argument("--steps", type=int, default=30, help="replayed steps per block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None, help="write the result here as well as to stdout")
    ap.add_argument("--from-json", default=None, help="a recorded result: nothing is measured")
    ap.add_argument("--write-docs", action="store_true", help="put the figures into DESIGN.md and README.md")
    args = ap.parse_args(argv)
    if args.from_json:
        r = json.load(open(args.from_json))
    else:
        r = measure(args)
        if args.json:
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            json.dump(r, open(args.json, "w"), indent=1)
    print(json.dumps({k: v for k, v in r.items()}))
    print(sentence(r))
    if args.write_docs:
        write_docs(r)
    return 0


if __name__ == "__main__":
    sys.exit(main())
