"""What a KL schedule with free bits (ConvolutionalMulVAE.set_kl_schedule) costs per replayed step, measured.

    python scripts/kl_schedule_cost.py [--batch 64] [--frames 128] [--rounds 8] [--steps 30] --json kl_sched_cost.json   (on the GPU)
    python scripts/kl_schedule_cost.py --from-json kl_sched_cost.json --write-docs                                       (anywhere)

Two trainers of the flagship workload (B = 64 / T = 128, fp32x3) in ONE process, one with the feature off and one with a
linear ramp long enough that the weight changes before EVERY step, free bits on; each replays its own captured hipGraph on
the same batch.  After a warm-up of both they are timed in alternating blocks of `--steps` steps (off, on, off, on, ...; a
host clock around a block that ends in a device synchronise), so that whatever else the host and the device are doing falls
on both alike.  Reported: the median block of either, the spread (min .. max) of the blocks, the difference of the medians,
and how many graphs the trainer with the schedule captured over all of its steps (its graph object is looked at after every
step).  The launch count of a step is the same with and without the feature, so the expectation is no difference outside
the spread; the times are recorded, not judged, and the comparison is the feature-off block of the same process.
--write-docs puts the figures of a recorded run between the `kl_sched_cost` markers of README.md."""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BEGIN, END = "<!-- kl_sched_cost:begin -->", "<!-- kl_sched_cost:end -->"


def measure(args):
    import torch
    import dvae_amd
    from dvae_amd import ops
    from dvae_amd.data import SyntheticPairs
    if not torch.cuda.is_available():
        raise SystemExit("kl_schedule_cost: no GPU; a time is measured on the device or not at all")
    dev = torch.device("cuda", torch.cuda.current_device())
    ops.set_compute_dtype(args.dtype)
    B, T = args.batch, args.frames
    x1, x2, spk = SyntheticPairs(B, T, n_speakers=10, seed=1234, device=dev).batch()
    total = args.warmup + args.rounds * args.steps
    graphs = []                             # the distinct graph objects of the trainer with the schedule, in order

    def look(w):
        if w._graph is not None and (not graphs or graphs[-1] is not w._graph):
            graphs.append(w._graph)

    def trainer(on):
        torch.manual_seed(1234)
        w = dvae_amd.ConvolutionalMulVAE("VCTK", T, 80, 32, 1e-4, 0.01, 500, False, batch_size=B, speaker_size=4,
                                         device=dev, latent_dim=32, mse_cof=10, kl_cof=10)
        w.model.train()
        if on:
            w.set_kl_schedule("linear", start=0.0, steps=total + 10, free_bits=args.free_bits)
        w.enable_graph(True)
        for _ in range(args.warmup):          # the first step is eager, the second captures, the rest replay
            w.step(x1, x2, spk, train=True)
            if on:
                look(w)
        assert w._graph is not None
        return w

    pair = {"off": trainer(False), "on": trainer(True)}
    weights = []

    def block(w, on):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            w.step_async(x1, x2, spk)
            if on:
                look(w)
                weights.append(w.kl_weight)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps

    times = {"off": [], "on": []}
    for _ in range(args.rounds):
        for name in ("off", "on"):
            times[name].append(block(pair[name], name == "on"))
    ops.lstm_pers_check()
    w = pair["on"]
    aux = w.kl_aux.tolist()

    def summary(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "blocks_ms": v}

    off, on = summary(times["off"]), summary(times["on"])
    return {"device": torch.cuda.get_device_name(dev), "batch": B, "frames": T, "dtype": args.dtype, "free_bits": args.free_bits,
            "rounds": args.rounds, "steps_per_block": args.steps, "warmup_steps": args.warmup,
            "step_off": off, "step_on": on, "difference_ms": on["median_ms"] - off["median_ms"],
            "graphs_captured": len(graphs), "steps_with_schedule": total, "optimizer_steps": w.optimizer.t,
            "distinct_weights_in_blocks": len(set(weights)), "timed_steps": len(weights),
            "last_weight": weights[-1], "device_weight": w._kl_coef[1].item(), "free_dims_last_step": aux[2:4]}


def sentence(r):
    off, on = r["step_off"], r["step_on"]
    d = r["difference_ms"]
    noise = max(off["max_ms"] - off["min_ms"], on["max_ms"] - on["min_ms"])
    verdict = (f"inside the spread of the blocks ({noise:.3f} ms)" if abs(d) <= noise else
               f"outside the spread of the blocks ({noise:.3f} ms)")
    return (f"Measured (`scripts/kl_schedule_cost.py`, one MI355X, one process, B = {r['batch']} / T = {r['frames']}, {r['dtype']}, "
            f"{r['rounds']} alternating blocks of {r['steps_per_block']} replayed steps each): "
            f"{off['median_ms']:.3f} ms per step with the feature off ({off['min_ms']:.3f} .. {off['max_ms']:.3f}), "
            f"{on['median_ms']:.3f} ms with a linear ramp and free bits of {r['free_bits']} nats on "
            f"({on['min_ms']:.3f} .. {on['max_ms']:.3f}): a difference of {d:+.3f} ms, {verdict}.  The weight took "
            f"{r['distinct_weights_in_blocks']} distinct values over the {r['timed_steps']} timed steps; the trainer captured "
            f"{r['graphs_captured']} graph over all {r['steps_with_schedule']} steps it ran with the schedule on.  "
            "The times are recorded, not judged.")


def write_docs(r):
    text = BEGIN + "\n" + sentence(r) + "\n" + END
    path = os.path.join(ROOT, "README.md")
    doc = open(path).read()
    if BEGIN not in doc or END not in doc:
        raise SystemExit(f"kl_schedule_cost: README.md has no {BEGIN} ... {END} block")
    doc = re.sub(re.escape(BEGIN) + ".*?" + re.escape(END), lambda _: text, doc, flags=re.S)
    open(path, "w").write(doc)
    print("kl_schedule_cost: wrote the figures into README.md")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--dtype", default="fp32x3")
    ap.add_argument("--free-bits", type=float, default=0.05, help="nats per dimension of the trainer with the schedule")
    ap.add_argument("--rounds", type=int, default=8, help="alternating blocks per variant")
    ap.add_argument("--steps", type=int, default=30, help="replayed steps per block")
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
    print(json.dumps({k: v for k, v in r.items()}))
    print(sentence(r))
    if args.write_docs:
        write_docs(r)
    return 0


if __name__ == "__main__":
    sys.exit(main())
