"""GPU box: the four launches of the latent map (dvae_amd.latent_map) timed with device events at N in
{4096, 32768} x D in {4, 28, 32} (seeded normal points, perplexity 30, a normal y of unit scale), and the wall time of a whole
750-iteration LatentMap.map at both sizes (D = 32).  Per figure: 3 warm-up launches, then `reps` launches timed one by one;
min and median in ms.  dvae_tsne_affinities is timed as one launch of the whole search (its passes are inside the kernel).
Prints one JSON line.  --write-docs FILE puts the figures of a recorded line (no GPU needed) between the latent_map_cost
markers of README.md.  The times are recorded, not judged: there is no earlier version."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

NS, DS, PERPLEXITY = (4096, 32768), (4, 28, 32), 30.0
BEGIN, END = "<!-- latent_map_cost:begin -->", "<!-- latent_map_cost:end -->"


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(float(np.min(ms)), 3), round(float(np.median(ms)), 3)


def main(reps=10):
    import dvae_amd  # noqa: F401
    from dvae_amd import latent_map
    from dvae_amd._lib import check, lib, ptr, stream
    if not torch.cuda.is_available():
        sys.exit("latent_map_cost: no GPU (a time comes from the MI355X or not at all)")
    dev = torch.device("cuda")
    lm = latent_map.LatentMap(dev)
    res = dict(reps=reps, perplexity=PERPLEXITY, shapes=[], maps=[])
    for D in DS:
        for N in NS:
            rs = np.random.RandomState(N + D)
            x = torch.from_numpy(rs.randn(N, D).astype(np.float32)).to(dev)
            y = torch.from_numpy(rs.randn(N, 2).astype(np.float32)).to(dev)
            grp = torch.from_numpy((np.arange(N) // 8).astype(np.int32)).to(dev)
            aff = lm.affinities(x, PERPLEXITY)
            steps = aff["steps"].cpu().numpy()
            d2min, arg = torch.empty(N, device=dev), torch.empty(N, device=dev, dtype=torch.int32)
            outs = [torch.empty(N, device=dev) for _ in range(3)] + [torch.empty(N, device=dev, dtype=torch.int32)]
            rows = torch.empty(N, 8, device=dev)
            upd, gains, kl = torch.zeros_like(y), torch.ones_like(y), torch.zeros(1, device=dev, dtype=torch.float64)
            h = lib()
            fig = dict(N=N, D=D, pairs=N * N, search_passes=int(steps.max()), unconverged=int((steps < 0).sum()))
            for name, fn in (
                ("nn", lambda: check(h.dvae_tsne_nn(ptr(x), D, N, D, ptr(grp), 0, N, ptr(d2min), ptr(arg), stream()), "nn")),
                ("affinities", lambda: check(h.dvae_tsne_affinities(ptr(x), D, N, D, ptr(aff["d2min"]), PERPLEXITY, 64, 0, N,
                                                                    *(ptr(o) for o in outs), stream()), "affinities")),
                ("forces", lambda: check(h.dvae_tsne_forces(ptr(x), D, N, D, ptr(aff["beta"]), ptr(aff["d2min"]),
                                                            ptr(aff["lnz"]), ptr(y), 0, 0, N, ptr(rows), stream()), "forces")),
                ("forces_kl", lambda: check(h.dvae_tsne_forces(ptr(x), D, N, D, ptr(aff["beta"]), ptr(aff["d2min"]),
                                                               ptr(aff["lnz"]), ptr(y), 1, 0, N, ptr(rows), stream()), "forces")),
                ("update", lambda: check(h.dvae_tsne_update(ptr(rows), N, ptr(y), ptr(upd), ptr(gains), 200.0, 0.8, 1.0,
                                                            ptr(kl), stream()), "update")),
            ):
                fig[name + "_min_ms"], fig[name + "_median_ms"] = timed(fn, reps)
            assert bool(torch.isfinite(rows).all())
            res["shapes"].append(fig)
    for N in NS:
        rs = np.random.RandomState(N)
        x = rs.randn(N, 32).astype(np.float32)
        spk = (np.arange(N) * 16 // N).astype(np.int32)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = lm.map(x, spk, np.arange(N) // 8)
        res["maps"].append(dict(N=N, D=32, iters=750, wall_s=round(time.perf_counter() - t0, 3), kl=r["kl"],
                                unconverged=r["unconverged"]))
    print(json.dumps(res))


def write_docs(path):
    res = json.loads(open(path).read().strip().splitlines()[-1])
    parts = []
    for s in res["shapes"]:
        parts.append(f"N = {s['N']}, D = {s['D']}: nn {s['nn_min_ms']:.3f} / {s['nn_median_ms']:.3f}, affinities "
                     f"{s['affinities_min_ms']:.3f} / {s['affinities_median_ms']:.3f} ({s['search_passes']} passes), forces "
                     f"{s['forces_min_ms']:.3f} / {s['forces_median_ms']:.3f} ({s['pairs'] / s['forces_min_ms'] * 1e-6:.1f} G "
                     f"pairs/s), forces with the KL sums {s['forces_kl_min_ms']:.3f} / {s['forces_kl_median_ms']:.3f}, update "
                     f"{s['update_min_ms']:.3f} / {s['update_median_ms']:.3f} ms")
    maps = "; ".join(f"N = {m['N']}: {m['wall_s']:.2f} s" for m in res["maps"])
    text = (f"Measured (`scripts/latent_map_cost.py`, one MI355X, device events, 3 warm-up launches then the minimum / median "
            f"of {res['reps']} launches timed one by one; the perplexity search is one launch of all its passes; seeded normal "
            f"points, perplexity {res['perplexity']:g}): " + "; ".join(parts)
            + f".  A whole 750-iteration `LatentMap.map` at D = 32 (wall clock, the searches, the descent, the three "
              f"nearest-neighbour launches and the downloads): {maps}.  The times are recorded, not judged: there is no earlier "
              f"version to compare with.")
    readme = os.path.join(ROOT, "README.md")
    doc = open(readme).read()
    i, j = doc.index(BEGIN) + len(BEGIN), doc.index(END)
    open(readme, "w").write(doc[:i] + "\n" + text + "\n" + doc[j:])


if __name__ == "__main__":
    if "--write-docs" in sys.argv[1:]:
        write_docs(sys.argv[sys.argv.index("--write-docs") + 1])
    else:
        main()
