"""GPU box: the speaker-identity probe (dvae_amd.probe) -- at rows = 4096 and classes = 109 and 1000 the ms
per call of the fused softmax cross-entropy (dvae_softmax_ce: loss, arg-max, sums AND the gradient of the logits, two
launches) next to torch.nn.functional.cross_entropy forward plus backward on the same tensors (the only path there was
before the kernel), both from HIP events around `reps` calls, with the two alternating in `rounds` rounds; the kernel's
algorithmic bytes over its time; and the seconds of one `fit` epoch on 100 000 x 28 synthetic features with 109 speakers
(minibatches of 4096: two Linear layers forward and backward, the loss kernel, one Adam launch each).  Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import dvae_amd  # noqa: F401
from dvae_amd import ops, probe as pr
from dvae_amd._lib import lib, ptr, stream


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


def ce_case(rows, classes, reps=200, rounds=5):
    ld = pr.pad_width(classes)
    rs = np.random.RandomState(classes)
    x = torch.from_numpy((rs.randn(rows, ld) * 3.0).astype(np.float32)).cuda()
    lab = torch.from_numpy(rs.randint(0, classes, rows).astype(np.int32)).cuda()
    lab64 = lab.long()
    d = torch.empty_like(x)
    row_loss = torch.empty(rows, device="cuda")
    row_pred = torch.empty(rows, device="cuda", dtype=torch.int32)
    out = torch.empty(4, device="cuda")

    def hip():
        rc = lib().dvae_softmax_ce(ptr(x), ptr(lab), ptr(d), ptr(row_loss), ptr(row_pred), ptr(out), rows, classes, ld,
                                   1.0 / rows, stream())
        assert rc == 0, rc

    xa = x[:, :classes].contiguous().requires_grad_(True)

    def aten():
        xa.grad = None
        torch.nn.functional.cross_entropy(xa, lab64).backward()

    hip_ms, aten_ms = [], []
    for _ in range(rounds):
        hip_ms.append(timed(hip, reps))
        aten_ms.append(timed(aten, reps))
    hip()
    aten()
    torch.cuda.synchronize()
    err = float((d[:, :classes] - xa.grad).abs().max())
    best = min(hip_ms)
    return dict(rows=rows, classes=classes, ld=ld, hip_ms=round(best, 5), hip_ms_rounds=[round(v, 5) for v in hip_ms],
                aten_ms=round(min(aten_ms), 5), aten_ms_rounds=[round(v, 5) for v in aten_ms],
                hip_gb_per_s=round(2.0 * rows * ld * 4 / best / 1e6, 1), max_grad_diff_to_aten=err,
                loss_hip=float(out[3]), loss_aten=float(torch.nn.functional.cross_entropy(xa.detach(), lab64)))


def fit_epoch(n=100000, dim=28, speakers=109):
    rs = np.random.RandomState(1)
    y = rs.randint(0, speakers, n).astype(np.int32)
    x = torch.from_numpy((rs.randn(speakers, dim)[y] + rs.randn(n, dim)).astype(np.float32)).cuda()
    p = pr.SpeakerProbe(dim, speakers, seed=0)
    p.fit(x, y, epochs=1)             # warm-up: code objects, slabs, workspaces
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = p.fit(x, y, epochs=2)    # ends in the epoch's host read of the loss
    torch.cuda.synchronize()
    return dict(fit_rows=n, fit_dim=dim, fit_speakers=speakers, fit_epoch_s=round((time.perf_counter() - t0) / 2, 4),
                fit_loss=round(losses[-1], 4), fit_accuracy=round(p.evaluate(x, y)["accuracy"], 4))


def main():
    res = dict(softmax_ce=[ce_case(4096, 109), ce_case(4096, 1000)], compute_dtype=ops.get_compute_dtype())
    res.update(fit_epoch())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
