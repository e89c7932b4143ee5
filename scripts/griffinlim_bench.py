"""GPU box: the Griffin-Lim inverse (frontend.MelInverter) on 64 utterances x 4 s, 32 iterations: ms per batch (mel ->
waveform, solve included), ms per Griffin-Lim iteration, the share of the two DFT contractions, and the float64 CPU
restatement (tests/test_griffinlim.py) on one utterance.  Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import dvae_amd  # noqa: F401
from dvae_amd.frontend import MelFrontend, MelInverter
from dvae_amd.packed import pinned_gemm


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main(n_utt=64, seconds=4.0, n_iter=32, reps=5):
    from test_griffinlim import griffin_lim, linear_magnitude, signal
    fe, inv = MelFrontend(), MelInverter(n_iter=n_iter)
    n = int(seconds * fe.sr)
    mels = fe.melspectrogram_batch([signal(n, i % 7 + 1) for i in range(n_utt)])
    rows = sum(m.shape[1] for m in mels)
    g = torch.Generator(device="cuda")
    batch_ms = timed(lambda: (g.manual_seed(0), inv.waveform_batch(mels, generator=g)), reps)
    solve_ms = timed(lambda: inv.linear_magnitude_batch(mels), reps)
    mags = inv.linear_magnitude_batch(mels)
    gl0_ms = timed(lambda: inv.griffinlim_batch(mags, n_iter=0, init="zeros"), reps)
    gl_ms = timed(lambda: inv.griffinlim_batch(mags, n_iter=n_iter, init="zeros"), reps)
    per_iter = (gl_ms - gl0_ms) / n_iter
    # the two contractions of one iteration alone
    X = torch.randn(rows, 2 * inv.nbp, device="cuda")
    y = torch.empty(rows, inv.fsize, device="cuda")
    R = torch.empty(rows, 2 * inv.nbp, device="cuda")
    gemm_ms = timed(lambda: (pinned_gemm(X, inv.inv_basis, y, 2 * inv.nbp), pinned_gemm(y, inv.dft_basis, R, inv.fsize)), 20)
    flop_iter = 2.0 * rows * inv.fsize * (2 * inv.nbp) * 2
    mel0 = mels[0].cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    S = linear_magnitude(mel0, inv.nnls_iter)
    griffin_lim(S, 2 * np.pi * np.random.RandomState(0).random_sample((S.shape[0], inv.nb)), n_iter)
    cpu_ms = 1e3 * (time.perf_counter() - t0)
    print(json.dumps(dict(utterances=n_utt, seconds=seconds, rows=rows, n_iter=n_iter, batch_ms=round(batch_ms, 3),
                          solve_ms=round(solve_ms, 3), ms_per_iteration=round(per_iter, 4),
                          contraction_ms_per_iteration=round(gemm_ms, 4),
                          contraction_share=round(gemm_ms / per_iter, 3) if per_iter > 0 else None,
                          contraction_tflops=round(flop_iter / gemm_ms / 1e9, 1), gflop_per_iteration=round(flop_iter / 1e9, 1),
                          cpu_fp64_one_utterance_ms=round(cpu_ms, 1))))


if __name__ == "__main__":
    main()
