"""What the smoothing penalty (ConvolutionalMulVAE.set_smoothing_penalty) costs per replayed step, measured.

    python scripts/msloss_cost.py [--batch 64] [--frames 128] [--rounds 8] [--steps 30] --json msloss_cost.json   (on the GPU)
    python scripts/msloss_cost.py --from-json msloss_cost.json --write-docs                                       (anywhere)

Two trainers of the flagship workload (B = 64 / T = 128, fp32x3) in ONE process, one with the feature off and one with both
weights on and a warm-up long enough that they change before EVERY step; each replays its own captured hipGraph on the same
batch.  "Off" launches what a trainer without the feature launches, so the off blocks are the baseline.  After a warm-up of both
they are timed in alternating blocks of `--steps` steps (off, on, off, on, ...; a host clock around a block that ends in a
device synchronise), so that whatever else the host and the device are doing falls on both alike.  Then the feature's own
launches are timed alone with device events on the step's shapes (y [2 B, 80, T], the default window): the two forward launches
(dvae_msloss_fwd), the one backward launch (dvae_msloss_bwd) and the one gradient sum of ops.fanout (dvae_sum_f32), each as the
median of `--reps` launches.  Reported: the median block of either variant, the spread of the blocks, the difference of the
medians, the launches' own times, how many graphs the trainer with the feature captured, and the device activities of one eager
step with and without (torch's profiler).  The times are recorded, not judged: the only expectation is that the added time is
what four small launches cost.
--write-docs puts the figures of a recorded run between the `msloss_cost` markers of README.md."""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BEGIN, END = "<!-- msloss_cost:begin -->", "<!-- msloss_cost:end -->"


def launches_alone(dev, N, C, T, reps):
    """median device time in microseconds of the feature's launches alone, between two events on the stream"""
    import torch
    from dvae_amd import ops
    from dvae_amd._lib import check, lib, ptr, stream
    L_ = lib()
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    y = torch.rand((N, C, T), device=dev, generator=g)
    x1, x2 = (torch.rand((N // 2, C, T), device=dev, generator=g) for _ in range(2))
    D = ops.msloss_window(T)
    tw = ops.msloss_twiddle(D, dev)
    w = torch.tensor([1.0, 1.0], device=dev)
    stats, pen = torch.empty(5, device=dev), torch.empty((), device=dev)
    ws = torch.empty(L_.dvae_msloss_ws_bytes(N, C) // 8, device=dev, dtype=torch.float64)
    dy, other, out = (torch.empty((N, C, T), device=dev) for _ in range(3))
    other.zero_()

    def fwd():
        check(L_.dvae_msloss_fwd(ptr(y), ptr(x1), ptr(x2), N // 2, C, T, D, 0.003, ptr(tw), ptr(w), ptr(stats), ptr(pen), ptr(ws),
                                 stream()), "fwd")

    def bwd():
        check(L_.dvae_msloss_bwd(ptr(y), ptr(x1), ptr(x2), N // 2, C, T, D, 0.003, ptr(tw), ptr(w), None, ptr(ws), ptr(dy),
                                 stream()), "bwd")

    def fan():
        check(L_.dvae_sum_f32(ptr(dy), ptr(other), None, ptr(out), N * C * T, stream()), "sum")

    res = {}
    for name, fn in (("fwd_two_launches_us", fwd), ("bwd_one_launch_us", bwd), ("fanout_sum_us", fan)):
        for _ in range(5):
            fn()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(1e3 * a.elapsed_time(b))
        res[name] = statistics.median(ts)
    return res


def launch_counts(dev, x1, x2, spk, B, T, weight):
    """device activities (kernels, copies, fills) of ONE eager step with the feature off and on, counted by torch's profiler;
    None where the profiler gives nothing"""
    import torch
    import dvae_amd
    from torch.profiler import ProfilerActivity, profile
    out = {}
    for name in ("off", "on"):
        torch.manual_seed(1234)
        w = dvae_amd.ConvolutionalMulVAE("VCTK", T, 80, 32, 1e-4, 0.01, 500, False, batch_size=B, speaker_size=4,
                                         device=dev, latent_dim=32, mse_cof=10, kl_cof=10)
        w.model.train()
        if name == "on":
            w.set_smoothing_penalty(weight, weight)
        for _ in range(2):
            w.step(x1, x2, spk, train=True)
        try:
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                w.step_async(x1, x2, spk)
                torch.cuda.synchronize()
            evs = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
            names = [e.name for e in evs]
            out[name] = {"device_activities": len(names),
                         "msloss_kernels": sum("msloss_" in n for n in names),
                         "copies_and_fills": sum(("memcpy" in n.lower()) or ("memset" in n.lower()) for n in names)}
        except Exception as e:      # a count is measured or it is not reported
            out[name] = None
            out["error"] = repr(e)[:200]
        del w
    return out


def measure(args):
    import torch
    import dvae_amd
    from dvae_amd import ops
    from dvae_amd.data import SyntheticPairs
    if not torch.cuda.is_available():
        raise SystemExit("msloss_cost: no GPU; a time is measured on the device or not at all")
    dev = torch.device("cuda", torch.cuda.current_device())
    ops.set_compute_dtype(args.dtype)
    B, T = args.batch, args.frames
    x1, x2, spk = SyntheticPairs(B, T, n_speakers=10, seed=1234, device=dev).batch()
    total = args.warmup + args.rounds * args.steps
    graphs = []

    def look(w):
        if w._graph is not None and (not graphs or graphs[-1] is not w._graph):
            graphs.append(w._graph)

    def trainer(on):
        torch.manual_seed(1234)
        w = dvae_amd.ConvolutionalMulVAE("VCTK", T, 80, 32, 1e-4, 0.01, 500, False, batch_size=B, speaker_size=4,
                                         device=dev, latent_dim=32, mse_cof=10, kl_cof=10)
        w.model.train()
        if on:
            w.set_smoothing_penalty(args.weight, args.weight, warmup_steps=total + 10)
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
                weights.append(w.smooth_weights)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps

    times = {"off": [], "on": []}
    for _ in range(args.rounds):
        for name in ("off", "on"):
            times[name].append(block(pair[name], name == "on"))
    ops.lstm_pers_check()
    w = pair["on"]

    def summary(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "blocks_ms": v}

    off, on = summary(times["off"]), summary(times["on"])
    alone = launches_alone(dev, 2 * B, 80, T, args.reps)
    del pair
    counts = launch_counts(dev, x1, x2, spk, B, T, args.weight)
    return {"device": torch.cuda.get_device_name(dev), "batch": B, "frames": T, "dtype": args.dtype, "weight": args.weight,
            "rounds": args.rounds, "steps_per_block": args.steps, "warmup_steps": args.warmup,
            "step_off": off, "step_on": on, "difference_ms": on["median_ms"] - off["median_ms"],
            "graphs_captured": len(graphs), "steps_with_feature": total, "optimizer_steps": w.optimizer.t,
            "distinct_weights_in_blocks": len(set(weights)), "timed_steps": len(weights),
            "device_weights": w._smooth_coef.tolist(), "smooth_aux_last_step": w.smooth_aux.tolist(),
            "window": w.smooth_cfg["window"], "alone": alone,
            "reps": args.reps, "eager_step_launches": counts}


def sentence(r):
    off, on, al = r["step_off"], r["step_on"], r["alone"]
    d = r["difference_ms"]
    noise = max(off["max_ms"] - off["min_ms"], on["max_ms"] - on["min_ms"])
    verdict = (f"inside the spread of the blocks ({noise:.3f} ms)" if abs(d) <= noise else
               f"outside the spread of the blocks ({noise:.3f} ms)")
    own = al["fwd_two_launches_us"] + al["bwd_one_launch_us"] + al["fanout_sum_us"]
    return (f"Measured (`scripts/msloss_cost.py`, one MI355X, one process, B = {r['batch']} / T = {r['frames']}, {r['dtype']}, "
            f"{r['rounds']} alternating blocks of {r['steps_per_block']} replayed steps each): "
            f"{off['median_ms']:.3f} ms per step with the feature off ({off['min_ms']:.3f} .. {off['max_ms']:.3f}), "
            f"{on['median_ms']:.3f} ms with both weights on and a warm-up that changes them before every step "
            f"({on['min_ms']:.3f} .. {on['max_ms']:.3f}): a difference of {d:+.3f} ms, {verdict}.  The feature's launches alone, "
            f"between device events on y [{2 * r['batch']}, 80, {r['frames']}] with windows of {r['window']} frames (median of "
            f"{r['reps']}): the two forward launches "
            f"{al['fwd_two_launches_us']:.1f} us, the backward launch {al['bwd_one_launch_us']:.1f} us, one gradient sum of "
            f"`ops.fanout` {al['fanout_sum_us']:.1f} us: {own:.1f} us together.  The weights took "
            f"{r['distinct_weights_in_blocks']} distinct values over the {r['timed_steps']} timed steps; the trainer captured "
            f"{r['graphs_captured']} graph over all {r['steps_with_feature']} steps it ran with the feature on.  "
            + counted(r) + "The times are recorded, not judged.")


def counted(r):
    c = r.get("eager_step_launches") or {}
    if not c.get("off") or not c.get("on"):
        return "The launches of a step were **not counted** on the device (the profiler gave nothing); by construction the feature adds four.  "
    a, b = c["off"]["device_activities"], c["on"]["device_activities"]
    return (f"One eager step is {a} device activities (kernels, copies, fills; torch's profiler) with the feature off and {b} "
            f"with it on ({b - a:+d}, {c['on']['msloss_kernels']} of them the penalty's own kernels).  ")


def write_docs(r):
    text = BEGIN + "\n" + sentence(r) + "\n" + END
    path = os.path.join(ROOT, "README.md")
    doc = open(path).read()
    if BEGIN not in doc or END not in doc:
        raise SystemExit(f"msloss_cost: README.md has no {BEGIN} ... {END} block")
    doc = re.sub(re.escape(BEGIN) + ".*?" + re.escape(END), lambda _: text, doc, flags=re.S)
    open(path, "w").write(doc)
    print("msloss_cost: wrote the figures into README.md")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--dtype", default="fp32x3")
    ap.add_argument("--weight", type=float, default=1.0, help="both weights of the trainer with the feature")
    ap.add_argument("--rounds", type=int, default=8, help="alternating blocks per variant")
    ap.add_argument("--steps", type=int, default=30, help="replayed steps per block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200, help="launches per figure of the feature's launches alone")
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
