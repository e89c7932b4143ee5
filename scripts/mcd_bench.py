"""GPU box: mel-cepstral distortion (dvae_amd.evaluate) -- for 256 pairs of 4 s synthetic 16 kHz utterances (harmonic tones
of varied pitch and noise level) the ms of the feature pass per call (both sides, 512 utterances, one packed batch; from
host arrays, and from device tensors: the GPU passes without the host packing and upload), of the DTW kernel alone on
prepared device tables, and of the whole mcd_batch per call (host packing, table uploads and read-backs included); and the
float64 numpy restatement (tests/test_mcd.py: features of both sides + DTW) on one pair.  Prints one JSON line.
With --f0 the line also carries, measured in the same call: f0_viterbi_ms (the F0 tracker's launch for the
512 utterances on the feature pass's buffers), dtw_f0_kernel_ms (the DTW kernel carrying the log-F0 payload, next to
dtw_kernel_ms), mcd_batch_f0_ms (mcd_batch(f0=True) per call) and mean_lf0_rmse_cents."""
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
from dvae_amd import evaluate as ev
from dvae_amd._lib import lib, ptr, stream
from test_mcd import dtw_ref, features_ref, harmonic


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


def main(pairs=256, seconds=4.0, reps=5, f0=False):
    rs = np.random.RandomState(0)
    n = int(16000 * seconds)
    conv = [harmonic(n, float(rs.uniform(80, 300)), seed=2 * i, snr_db=float(rs.uniform(10, 30))) for i in range(pairs)]
    ref = [harmonic(n, float(rs.uniform(80, 300)), seed=2 * i + 1, snr_db=float(rs.uniform(10, 30))) for i in range(pairs)]
    fe = ev.MelCepstrum()
    features_ms = timed(lambda: fe.packed(conv + ref), reps)
    on_device = [torch.from_numpy(w).cuda() for w in conv + ref]
    features_device_ms = timed(lambda: fe.packed(on_device), reps)
    out = fe.packed(conv + ref)
    table, count = out["table"], out["count"]
    P = pairs
    tab = np.ascontiguousarray(np.stack([table[:P, 0], count[:P], table[P:, 0], count[P:]], axis=1), dtype=np.int64)
    tab_d = torch.from_numpy(tab).cuda()
    cost = torch.empty(P, device="cuda", dtype=torch.float64)
    length = torch.empty(P, device="cuda", dtype=torch.int64)
    feats = out["feats"]

    def dtw():
        rc = lib().dvae_dtw_batch(ptr(feats), ptr(feats), ptr(tab_d), tab.ctypes.data, P, ptr(cost), ptr(length), stream())
        assert rc == 0, rc
    dtw_kernel_ms = timed(dtw, reps)
    mcd_batch_ms = timed(lambda: ev.mcd_batch(conv, ref, features=fe), reps)
    res = ev.mcd_batch(conv, ref, features=fe)
    t0 = time.perf_counter()
    fx, fy = features_ref(conv[0]), features_ref(ref[0])
    c, l = dtw_ref(fx["mc"][fx["voiced"], :ev.DIM], fy["mc"][fy["voiced"], :ev.DIM])
    f64_one_pair_s = time.perf_counter() - t0
    cells = float(np.sum(count[:P].astype(np.float64) * count[P:]))
    extra = {}
    if f0:
        rows = int(table[:, 1].sum())
        segs = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int64)).cuda()
        bufs = fe.f0_viterbi(out["r"], out["voiced"], segs, 2 * P, rows)
        f0_viterbi_ms = timed(lambda: fe.f0_viterbi(out["r"], out["voiced"], segs, 2 * P, rows, out=bufs), reps)
        sse = torch.empty(P, device="cuda", dtype=torch.float64)
        lf0v = bufs["lf0v"]

        def dtw_f0():
            rc = lib().dvae_dtw_batch_f0(ptr(feats), ptr(feats), ptr(lf0v), ptr(lf0v), ptr(tab_d), tab.ctypes.data, P,
                                         ptr(cost), ptr(length), ptr(sse), stream())
            assert rc == 0, rc
        dtw_f0_kernel_ms = timed(dtw_f0, reps)
        mcd_batch_f0_ms = timed(lambda: ev.mcd_batch(conv, ref, features=fe, f0=True), reps)
        res_f0 = ev.mcd_batch(conv, ref, features=fe, f0=True)
        extra = dict(f0_viterbi_ms=round(f0_viterbi_ms, 3), dtw_f0_kernel_ms=round(dtw_f0_kernel_ms, 3),
                     mcd_batch_f0_ms=round(mcd_batch_f0_ms, 3),
                     mean_lf0_rmse_cents=round(res_f0["mean_lf0_rmse_cents"], 3))
    print(json.dumps(dict(pairs=P, seconds=seconds, frames_per_utterance=int(table[0, 1]),
                          voiced_mean=float(count.mean()), dtw_cells=cells, features_ms=round(features_ms, 3),
                          features_device_ms=round(features_device_ms, 3),
                          dtw_kernel_ms=round(dtw_kernel_ms, 3), dtw_gcells_per_s=round(cells / dtw_kernel_ms / 1e6, 3),
                          mcd_batch_ms=round(mcd_batch_ms, 3), mean_mcd=round(res["mean_mcd"], 4),
                          f64_one_pair_s=round(f64_one_pair_s, 3), f64_one_pair_mcd=round(float(ev.mcd_from([c], [l])[0]), 4),
                          gpu_one_pair_mcd=round(float(res["mcd"][0]), 4), **extra)))


if __name__ == "__main__":
    main(f0="--f0" in sys.argv[1:])
