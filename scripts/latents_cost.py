"""GPU box: dvae_latent_lse (dvae_amd.latents) timed with device events on the report's global job alone,
{0, N, 0, N, 0}, at N in {4096, 32768} x D in {32, 64} (S = 4; seeded posteriors: mu ~ N(0, 1), lv ~ U(-3, 0)).  Per figure:
3 warm-up launches, then `--reps` launches timed one by one; min and median in ms, beside the number of exponentials the
launch takes, N N (D + 3).  Prints one JSON line.  --write-docs FILE puts the figures of a recorded line (no GPU needed)
between the latents_cost markers of README.md.  The times are recorded, not judged: there is no earlier version."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

NS, DS, S = (4096, 32768), (32, 64), 4
BEGIN, END = "<!-- latents_cost:begin -->", "<!-- latents_cost:end -->"


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
    from dvae_amd import latents
    from dvae_amd._lib import check, lib, ptr, stream
    if not torch.cuda.is_available():
        sys.exit("latents_cost: no GPU (a time comes from the MI355X or not at all)")
    dev = torch.device("cuda")
    rep = latents.LatentReport(dev)
    res = dict(reps=reps, S=S, shapes=[])
    for D in DS:
        for N in NS:
            rs = np.random.RandomState(N + D)
            t = rep.tables(rs.randn(N, D).astype(np.float32), rs.uniform(-3.0, 0.0, (N, D)).astype(np.float32),
                           rs.randn(N, D).astype(np.float32))
            jobs = np.array([[0, N, 0, N, 0]], np.int64)
            jd = torch.from_numpy(jobs).to(dev)
            out = torch.empty(N, D + 3, device=dev)

            def launch():
                check(lib().dvae_latent_lse(ptr(t["z"]), ptr(t["mu"]), ptr(t["a"]), ptr(t["h"]), D, D, S, ptr(jd),
                                            jobs.ctypes.data, 1, ptr(out), D + 3, stream()), "dvae_latent_lse")

            lo, med = timed(launch, reps)
            assert bool(torch.isfinite(out).all())
            res["shapes"].append(dict(N=N, D=D, min_ms=lo, median_ms=med, exponentials=N * N * (D + 3)))
    print(json.dumps(res))


def write_docs(path):
    res = json.loads(open(path).read().strip().splitlines()[-1])
    parts = [f"N = {s['N']}, D = {s['D']}: {s['min_ms']:.3f} / {s['median_ms']:.3f} ms for {s['exponentials']:.2e} exponentials "
             f"({s['exponentials'] / s['min_ms'] * 1e-6:.1f} G/s)" for s in res["shapes"]]
    text = (f"Measured (`scripts/latents_cost.py`, one MI355X, device events, 3 warm-up launches then the minimum / median of "
            f"{res['reps']} launches timed one by one; `dvae_latent_lse`, the global job {{0, N, 0, N, 0}} alone, S = "
            f"{res['S']}; a launch takes N N (D + 3) exponentials and about ten plain vector operations beside each): "
            + "; ".join(parts) + ".  The times are recorded, not judged: there is no earlier version to compare with.")
    readme = os.path.join(ROOT, "README.md")
    doc = open(readme).read()
    i, j = doc.index(BEGIN) + len(BEGIN), doc.index(END)
    open(readme, "w").write(doc[:i] + "\n" + text + "\n" + doc[j:])


if __name__ == "__main__":
    if "--write-docs" in sys.argv[1:]:
        write_docs(sys.argv[sys.argv.index("--write-docs") + 1])
    else:
        main()
