"""GPU box: the two kernels of the GMM-UBM speaker verification (dvae_amd.verify), timed with device events
on N = 2^20 frames of D = 23 coefficients in a [N, 24] buffer (col0 = 1, as MelCepstrum.packed leaves them), at K = 64 and
K = 256: dvae_gmm_estep (both launches; with and without the optional lse / gamma outputs) and dvae_gmm_score (the same
frames as 2048 utterances of 512 frames, M = 3 models).  Per figure: 3 warm-up calls, then `--reps` calls timed one by one;
min and median in ms.  Prints one JSON line.  --write-docs FILE puts the figures of a recorded line (no GPU needed) between
the verify_cost markers of README.md."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import dvae_amd  # noqa: F401
from dvae_amd import verify
from dvae_amd._lib import check, lib, ptr, stream
from dvae_amd.packed import upload

N, D, LD, COL0, UTT = 1 << 20, 23, 24, 1, 512
BEGIN, END = "<!-- verify_cost:begin -->", "<!-- verify_cost:end -->"


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


def model(rs, K):
    return verify.DiagGMM(rs.dirichlet(np.ones(K) * 5.0), rs.randn(K, D), rs.uniform(0.5, 1.5, (K, D)))


def main(reps=10):
    rs = np.random.RandomState(0)
    dev = torch.device("cuda")
    x = torch.randn(N, LD, device=dev, generator=torch.Generator(dev).manual_seed(0)) * 1.5
    segs = upload(np.stack([np.arange(0, N, UTT), np.full(N // UTT, UTT)], axis=1), dev, np.int64)
    L = lib()
    res = dict(frames=N, dim=D, utterances=N // UTT, models=3, reps=reps)
    for K in (64, 256):
        ms = [model(rs, K) for _ in range(3)]
        a, mu, prec = verify._device_tables(ms, dev)
        ws = torch.empty(int(L.dvae_gmm_ws_bytes(N, K, D)), device=dev, dtype=torch.uint8)
        stats = torch.empty(verify.stats_size(K, D), device=dev, dtype=torch.float64)
        lse = torch.empty(N, device=dev)
        gamma = torch.empty(N, K, device=dev)
        out = torch.empty(N // UTT, 3, device=dev, dtype=torch.float64)

        def estep(full):
            check(L.dvae_gmm_estep(ptr(x), LD, COL0, N, D, ptr(a), ptr(mu), ptr(prec), K, ptr(lse) if full else None,
                                   ptr(gamma) if full else None, ptr(ws), ptr(stats), stream()), "dvae_gmm_estep")

        def score():
            check(L.dvae_gmm_score(ptr(x), LD, COL0, D, ptr(segs), N // UTT, ptr(a), ptr(mu), ptr(prec), K, 3, ptr(out),
                                   stream()), "dvae_gmm_score")

        res[f"estep_k{K}_ms"] = timed(lambda: estep(False), reps)
        res[f"estep_outputs_k{K}_ms"] = timed(lambda: estep(True), reps)
        res[f"score_k{K}_ms"] = timed(score, reps)
        res[f"mean_ll_k{K}"] = round(float(stats[-1].item()) / N, 4)
    print(json.dumps(res))


def write_docs(path):
    res = json.loads(open(path).read().strip().splitlines()[-1])
    f = lambda k: f"{res[k][0]:.3f} ms (median {res[k][1]:.3f})"
    n, u = res["frames"], res["utterances"]
    text = (f"Measured (`scripts/verify_bench.py`, one MI355X, device events, 3 warm-up calls then the minimum of "
            f"{res['reps']} calls timed one by one; N = 2^20 frames, D = 23 read in place from a [N, 24] buffer): "
            f"`dvae_gmm_estep` (statistics only, both launches) {f('estep_k64_ms')} at K = 64 and {f('estep_k256_ms')} at "
            f"K = 256; with `lse` and `gamma` written {f('estep_outputs_k64_ms')} and {f('estep_outputs_k256_ms')}; "
            f"`dvae_gmm_score` (the same frames as {u} utterances of {n // u} frames under {res['models']} models) "
            f"{f('score_k64_ms')} and {f('score_k256_ms')}.")
    readme = os.path.join(ROOT, "README.md")
    doc = open(readme).read()
    i, j = doc.index(BEGIN) + len(BEGIN), doc.index(END)
    open(readme, "w").write(doc[:i] + "\n" + text + "\n" + doc[j:])


if __name__ == "__main__":
    if "--write-docs" in sys.argv[1:]:
        write_docs(sys.argv[sys.argv.index("--write-docs") + 1])
    else:
        main()
