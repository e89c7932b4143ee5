"""Child process of tests/test_hip_ddp.py: ONE rank on cuda:0 with the real RCCL backend ("nccl"), so that the
data-parallel step — ops.grad_ready_hook -> GradReducer (bucketed all-reduce issued from the autograd thread while the
HIP backward kernels are still being enqueued) -> FlatAdam(grad_scale) — runs on the HIP kernels.  Started as a FRESH
process: nothing has touched the GPU before init_process_group.  Prints one JSON line.

argv: <graph 0|1> <lr> <steps> [features]
features: both trainers run with the KL schedule and free bits, the factor penalty with its warm-up, gradient clipping at half the
first step's norm (measured by a throwaway trainer) and the weight average on — no adversary, which is refused under a reducer —
and the line gains `same` (torch.equal of the two trainers' state, name by name), the two host counters and the clip counters."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    use_graph, lr, steps = int(sys.argv[1]), float(sys.argv[2]), int(sys.argv[3])
    features = len(sys.argv) > 4 and sys.argv[4] == "features"
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", device_id=dev, rank=0, world_size=1)
    import dvae_amd
    from dvae_amd import ddp
    from oracle.fill import fill_state_dict, synthetic_eps, synthetic_pair     # deterministic weights / inputs only

    B, T = 4, 64

    def make(with_reducer, max_norm=None):
        w = dvae_amd.ConvolutionalMulVAE("VCTK", T, 80, 32, lr, 0.01, 500, False, batch_size=B, speaker_size=4,
                                         device=dev, latent_dim=32, mse_cof=10, kl_cof=10)
        w.model.load_state_dict(fill_state_dict(w.model.state_dict()))
        w.model.train()
        if max_norm is not None:
            w.set_kl_schedule("linear", start=1.0, steps=6, free_bits=0.05)
            w.set_factor_penalty(3.0, 1.5, warmup_steps=7)
            w.optimizer.set_grad_clip(max_norm)
            w.optimizer.set_ema(0.9)
        red = None
        if with_reducer:
            ddp.broadcast_parameters(w.optimizer.flat_p, list(w.model.buffers()))
            red = ddp.GradReducer(w.optimizer.flat_g, w.optimizer.names, w.optimizer.params, w.optimizer.offsets,
                                  mode=os.environ.get("DVAE_DDP_MODE", "all_reduce"),
                                  issue=os.environ.get("DVAE_DDP_ISSUE", "hook"))
            red.force = True                    # issue the collectives although world_size == 1
            w.attach_reducer(red)
            if use_graph:
                w.enable_graph(True, ddp=True)
        return w, red

    max_norm = None
    if features:
        probe, _ = make(False)
        probe.optimizer.set_grad_clip(float("inf"))
        probe.model.eps_override = synthetic_eps(B, seed=200)
        probe.step(*(t.cuda() for t in synthetic_pair(B, T, 100)), None, train=True)
        max_norm = probe.optimizer.grad_clip_stats()["norm"] / 2
        del probe
    a, _ = make(False, max_norm)
    b, red = make(True, max_norm)
    out = {"graph": use_graph, "lr": lr, "buckets": len(red.buckets), "losses_plain": [], "losses_ddp": []}
    for i in range(steps):
        x1, x2 = (t.cuda() for t in synthetic_pair(B, T, 100 + i))
        eps = synthetic_eps(B, seed=200 + i)
        a.model.eps_override = eps
        b.model.eps_override = eps
        out["losses_plain"].append(list(a.step(x1, x2, None, train=True)))
        out["losses_ddp"].append(list(b.step(x1, x2, None, train=True)))
    torch.cuda.synchronize()
    from dvae_amd import ops
    out["deterministic"] = bool(ops.deterministic())
    out["ddp_mode"] = red.mode
    out["graph_captured"] = b._graph is not None
    out["stats"] = red.stats
    out["views_intact"] = bool(a.optimizer.views_intact() and b.optimizer.views_intact())
    out["t"] = [a.optimizer.t, b.optimizer.t]
    # distance of the two parameter vectors (Adam's first updates are lr * sign(g): every gradient element that is zero
    # up to round-off moves its weight by +-lr independently in the two trainers, so the trajectories are not bitwise equal)
    out["param_dist_rel"] = float((a.optimizer.flat_p - b.optimizer.flat_p).double().norm() /
                                  a.optimizer.flat_p.double().norm())
    out["param_moved_rel"] = float(lr * steps * (a.optimizer.numel ** 0.5) / a.optimizer.flat_p.double().norm())
    ma, mb = a.optimizer.exp_avg, b.optimizer.exp_avg
    out["exp_avg_rel"] = float((ma - mb).norm() / ma.norm())
    if features:
        pairs = [(n, getattr(a.optimizer, n), getattr(b.optimizer, n)) for n in ("flat_p", "exp_avg", "exp_avg_sq", "ema", "clip_state")]
        pairs += [("kl_aux", a.kl_aux, b.kl_aux), ("factor_aux", a.factor_aux, b.factor_aux)]
        pairs += [("buffer " + n, u, v) for (n, u), (_, v) in zip(a.model.named_buffers(), b.model.named_buffers())]
        out["same"] = {n: bool(torch.equal(u, v)) for n, u, v in pairs}
        out["max_norm"] = max_norm
        out["step_k"] = [a._step_k, b._step_k]
        out["clipped"] = [a.optimizer.grad_clip_stats()["clipped"], b.optimizer.grad_clip_stats()["clipped"]]
        out["skipped"] = [a.optimizer.grad_clip_stats()["skipped"], b.optimizer.grad_clip_stats()["skipped"]]
    print("DDPCHILD " + json.dumps(out), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
