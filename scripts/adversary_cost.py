"""What the speaker adversary (ConvolutionalMulVAE.set_speaker_adversary) costs, measured.

    python scripts/adversary_cost.py [--batch 64] [--frames 128] [--rounds 8] [--steps 30] --json adversary_cost.json   (on the GPU)
    python scripts/adversary_cost.py --from-json adversary_cost.json --write-docs                                       (anywhere)

One process.  (1) Two trainers of the flagship workload (B = 64 / T = 128, fp32x3), one with the adversary off and one with it
on (weight 0.5, a warm-up long enough that the weight changes before every step); each replays its own captured hipGraph on
the same batch, timed in alternating blocks of `--steps` steps (a host clock around a block that ends in a device
synchronise).  The difference is recorded, not judged.  (2) At the step's shape R = 128, D = 28, H = 256, S = 109, forward
and backward of the classifier two ways, each as eager launches and as a replayed hipGraph of its own, timed with device events,
minimum and median of `--reps`: the two fused launches (ops.speaker_adversary: dvae_adv_rows, dvae_adv_params), and the same
arithmetic composed from ops.LinearFn x2 and ops.SoftmaxCeFn through autograd, as the project offered it before.  The fused
pair must take less time than the composed path; --write-docs says which way it went between the `adversary_cost` markers of
README.md."""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BEGIN, END = "<!-- adversary_cost:begin -->", "<!-- adversary_cost:end -->"
R_, D_, H_, S_ = 128, 28, 256, 109


def classifier_times(args, dev):
    """(fused, composed): {eager: {min_us, median_us}, graph: {...}} at R = 128, D = 28, H = 256, S = 109"""
    import torch
    from dvae_amd import ops
    from dvae_amd.adversary import SpeakerAdversary
    from dvae_amd.probe import SpeakerProbe
    torch.manual_seed(7)
    x = torch.randn(R_, D_, device=dev)
    labels = torch.randint(0, S_, (R_,), device=dev, dtype=torch.int32)
    adv = SpeakerAdversary(D_, S_, hidden=H_, seed=0, device=dev)
    coef = torch.full((1,), 0.5, device=dev)
    p = adv.params
    grads = tuple(p[k].grad for k in ("w1", "b1", "w2", "b2"))

    def fused():
        return ops.speaker_adversary(x, labels, p["w1"].detach(), p["b1"].detach(), p["w2"].detach(), p["b2"].detach(), coef,
                                     0, D_, grads)

    probe = SpeakerProbe(D_, S_, hidden=H_, seed=0, device=dev)
    xq = x.clone().requires_grad_(True)

    def composed():
        loss = probe.loss(xq, labels, R_)
        loss.backward()
        return loss

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        eager = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            eager.append(1e3 * a.elapsed_time(b))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        g.replay()
        torch.cuda.synchronize()
        graph = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            graph.append(1e3 * a.elapsed_time(b))
        s = lambda v: {"min_us": min(v), "median_us": statistics.median(v), "all_us": v}
        return {"eager": s(eager), "graph": s(graph)}

    return timed(fused), timed(composed)


def measure(args):
    import torch
    import dvae_amd
    from dvae_amd import ops
    from dvae_amd.data import SyntheticPairs
    if not torch.cuda.is_available():
        raise SystemExit("adversary_cost: no GPU; a time is measured on the device or not at all")
    dev = torch.device("cuda", torch.cuda.current_device())
    ops.set_compute_dtype(args.dtype)
    B, T = args.batch, args.frames
    x1, x2, spk = SyntheticPairs(B, T, n_speakers=S_, seed=1234, device=dev).batch()
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
            w.set_speaker_adversary(0.5, n_speakers=S_, hidden=H_, warmup_steps=total + 10)
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
                weights.append(w.adv_weight)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps

    times = {"off": [], "on": []}
    for _ in range(args.rounds):
        for name in ("off", "on"):
            times[name].append(block(pair[name], name == "on"))
    ops.lstm_pers_check()
    w = pair["on"]
    summary = lambda v: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "blocks_ms": v}
    off, on = summary(times["off"]), summary(times["on"])
    fused, composed = classifier_times(args, dev)
    return {"device": torch.cuda.get_device_name(dev), "batch": B, "frames": T, "dtype": args.dtype, "rounds": args.rounds,
            "steps_per_block": args.steps, "warmup_steps": args.warmup, "step_off": off, "step_on": on,
            "difference_ms": on["median_ms"] - off["median_ms"], "graphs_captured": len(graphs),
            "steps_with_adversary": total, "distinct_weights_in_blocks": len(set(weights)), "timed_steps": len(weights),
            "adv_out_last": w.adv_out.tolist(), "shape": [R_, D_, H_, S_], "reps": args.reps, "fused": fused, "composed": composed}


def sentence(r):
    off, on, d = r["step_off"], r["step_on"], r["difference_ms"]
    f, c = r["fused"], r["composed"]
    faster = f["graph"]["median_us"] < c["graph"]["median_us"] and f["eager"]["median_us"] < c["eager"]["median_us"]
    verdict = ("the fused pair takes less time than the composed path both ways" if faster else
               "the fused pair does NOT take less time than the composed path: the composed path should be shipped instead")
    R, D, H, S = r["shape"]
    return (f"Measured (`scripts/adversary_cost.py`, one MI355X, one process, B = {r['batch']} / T = {r['frames']}, {r['dtype']}, "
            f"{r['rounds']} alternating blocks of {r['steps_per_block']} replayed steps each): {off['median_ms']:.3f} ms per step "
            f"with the adversary off ({off['min_ms']:.3f} .. {off['max_ms']:.3f}), {on['median_ms']:.3f} ms with it on "
            f"({on['min_ms']:.3f} .. {on['max_ms']:.3f}): a difference of {d:+.3f} ms, recorded, not judged; the weight took "
            f"{r['distinct_weights_in_blocks']} distinct values over the {r['timed_steps']} timed steps under {r['graphs_captured']} "
            f"captured graph.  The classifier alone at R = {R}, D = {D}, H = {H}, S = {S}, forward and backward, device events, "
            f"minimum / median of {r['reps']}: the two fused launches {f['graph']['min_us']:.1f} / {f['graph']['median_us']:.1f} us "
            f"as a replayed graph and {f['eager']['min_us']:.1f} / {f['eager']['median_us']:.1f} us as eager launches; the same "
            f"arithmetic composed from `ops.LinearFn` x2 and `ops.SoftmaxCeFn` through autograd {c['graph']['min_us']:.1f} / "
            f"{c['graph']['median_us']:.1f} us as a replayed graph and {c['eager']['min_us']:.1f} / {c['eager']['median_us']:.1f} us "
            f"eager: {verdict}.  The two arms are the two ways the trainer could run the classifier, not the same arithmetic "
            f"to the bit: the composed path's contractions run in the process's compute mode ({r['dtype']}: fp32 results on "
            "the bf16 matrix pipe), the fused kernels are plain fp32 vector code.")


def write_docs(r):
    text = BEGIN + "\n" + sentence(r) + "\n" + END
    path = os.path.join(ROOT, "README.md")
    doc = open(path).read()
    if BEGIN not in doc or END not in doc:
        raise SystemExit(f"adversary_cost: README.md has no {BEGIN} ... {END} block")
    doc = re.sub(re.escape(BEGIN) + ".*?" + re.escape(END), lambda _: text, doc, flags=re.S)
    open(path, "w").write(doc)
    print("adversary_cost: wrote the figures into README.md")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--dtype", default="fp32x3")
    ap.add_argument("--rounds", type=int, default=8, help="alternating blocks per variant")
    ap.add_argument("--steps", type=int, default=30, help="replayed steps per block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="device-event timings of each classifier path")
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
