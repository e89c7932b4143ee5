"""`python -m dvae_amd.selftest [--rounds 200] [--device 0]` — does THIS GPU run the W_hh-resident persistent recurrences right?

The persistent LSTM launches (csrc/lstm_pers.hip) hand h[t] / dG[t] from workgroup to workgroup through write-through stores,
flags and L1-bypassing loads: a form that is measured valid on gfx950, not architecturally guaranteed, and in
rounds 4 and 5 one chip in fifty-nine showed wrong rows in a kernel form that every other chip ran 5 000 times without one.
Before a long training run on a new box, this runs every persistent kernel the product dispatches (default arithmetic: forward +
both backward forms at H = 512 and H = 1024; bf16 mode: H = 512 and H = 1024, at T = 48 and at the T = 512 of BASELINE configs[4]) for `--rounds` rounds while a second stream
streams 0 .. 4 GiB through HBM, and compares every output word with the one-launch-per-frame kernels of the same arithmetic and,
bit for bit, with the first persistent round; the bias gradients, which the persistent backward launch leaves per row group in
the dbias_part slabs as in training, against the column sums of that launch's own dgates.  Exit code 0: all equal; 1: a mismatch (the report names kernel, tensor, round,
frame and rows, and the GPU's KFD unique_id); a failing box should train with DVAE_LSTM_PERSISTENT=0.
"""
from __future__ import annotations

import argparse
import glob
import sys

import os
import torch


def gpu_unique_ids():
    """KFD unique_id of every GPU node the topology shows (no HIP call)."""
    out = []
    for path in sorted(glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties")):
        try:
            kv = dict(ln.split()[:2] for ln in open(path) if len(ln.split()) >= 2)
            if int(kv.get("simd_count", "0")) > 0:
                out.append(hex(int(kv.get("unique_id", "0"))))
        except Exception:
            pass
    return out


def _pass(mode, H, T, N, pers, seed=0):
    """forward + backward recurrence of one layer through the C ABI, with the descriptors and — persistent — the bias path of
    the product (ops._lstm_dir, ops._pers_fill; bias gradients stored per row group into the dbias_part slabs, as
    ops.pers_bias_slabs provides them); returns (gates, c, h, dgates, slabs): slabs [PERS_BIAS_SLABS, 4H], None for the
    per-frame launches, which leave no bias gradient"""
    from . import _lib, ops
    from .derived import lstm_local
    L, st = _lib.lib(), _lib.stream()
    bf = mode == _lib.MODE_BF16
    g = torch.Generator(device="cuda").manual_seed(1000 + seed)
    f = dict(device="cuda", dtype=torch.float32)
    sdt = torch.bfloat16 if bf else torch.float32
    w_hh = (torch.rand(4 * H, H, generator=g, **f) * 2 - 1) / H ** 0.5
    der = lstm_local(torch.zeros(4 * H, 64, **f), w_hh, torch.zeros(4 * H, **f), torch.zeros(4 * H, **f), mode)
    gates = torch.rand(T * N, 4 * H, generator=g, **f) * 2 - 1
    dh = (torch.rand(T * N, H, generator=g, **f) * 2 - 1) * 0.1
    h = torch.full((T * N, H), float("nan"), device="cuda", dtype=sdt)
    c = torch.empty(T * N, H, **f)
    dg = torch.full((T * N, 4 * H), float("nan"), device="cuda", dtype=sdt)
    dc = torch.empty(N, H, **f)
    part = torch.zeros(_lib.PERS_BIAS_SLABS, 4 * H, **f) if pers else None
    d, b = (_lib.LstmDir * 1)(), (_lib.LstmDir * 1)()
    common = dict(H=H, gates=gates, c_all=c, packed_mode=mode, state_bf16=bf)
    ops._lstm_dir(d[0], w_hh=w_hh, w_packed=der.pack_f, h_out=h, **common)
    ops._lstm_dir(b[0], w_hh=der.w_hh_t, w_packed=der.pack_b, dh_out=dh, dgates=dg, dc_ws=dc, **common)
    if pers:                             # (claims the device: one persistent launch at a time, as every product call site)
        ops._pers_fill(d[0], "cuda")
        ops._pers_fill(b[0], "cuda", part)
    _lib.check(L.dvae_lstm_seq_fwd(d, 1, T, N, H, H, st), "fwd")
    _lib.check(L.dvae_lstm_seq_bwd(b, 1, T, N, H, H, st), "bwd")
    if pers:
        ops.lstm_pers_check()
    return [t.float() for t in (gates, c, h, dg)] + [part]


def _bias_slabs_wrong(slabs, dgates, T, N, first=None):
    """What is wrong with the bias-gradient slabs of a persistent backward launch (None: nothing).  Held as
    tests/lstm_ref.py bias_check holds them: slabs of row groups the launch cannot have (>= ceil(N/16)) exactly zero, and the
    float64 sum over the slabs, per column, against the float64 column sum s of the launch's OWN dgates within
    gamma(T*N + 16) * sum|dG| + eps32 * |s|, gamma(n) = n eps32 / (1 - n eps32) — T*N fp32 additions in whatever order plus
    the 16 of the slab sum, and the rounding of the result; and bit for bit against the first good round (`first`)."""
    if not bool(torch.isfinite(slabs).all()):
        return "not finite"
    if bool((slabs[-(-N // 16):] != 0).any()):
        return f"a slab of a row group >= {-(-N // 16)}, which the launch does not have, is not zero"
    eps32, n = 2.0 ** -24, T * N + 16
    dg = dgates.double()
    s = dg.sum(0)
    bound = n * eps32 / (1.0 - n * eps32) * dg.abs_().sum(0) + eps32 * s.abs()
    err = (slabs.double().sum(0) - s).abs()
    if bool((err > bound).any()):
        j = int((err - bound).argmax())
        return f"column {j}: |sum of slabs - column sum of dgates| {float(err[j]):.3e} (bound {float(bound[j]):.3e})"
    if first is not None and not torch.equal(slabs, first):
        return "persistent rounds differ bitwise"
    return None


def run(rounds: int = 200, log=print) -> int:
    from . import _lib, ops
    if not torch.cuda.is_available():
        raise RuntimeError("dvae_amd.selftest needs the GPU it is to test")
    log(f"GPU unique_id(s): {gpu_unique_ids()}; device {torch.cuda.current_device()}: {torch.cuda.get_device_name()}")
    cases = [("fp32x3", _lib.MODE_F32X3, 1024, 64, 128, 2e-5), ("fp32x3", _lib.MODE_F32X3, 512, 64, 128, 2e-5),
             ("bf16", _lib.MODE_BF16, 1024, 48, 256, 2e-2), ("bf16", _lib.MODE_BF16, 1024, 48, 128, 2e-2),
             ("bf16", _lib.MODE_BF16, 512, 48, 128, 2e-2),
             # BASELINE configs[4]'s per-GPU shape: the 16-row bf16 forms over T = 512 frames
             ("bf16", _lib.MODE_BF16, 1024, 512, 128, 2e-2), ("bf16", _lib.MODE_BF16, 512, 512, 128, 2e-2)]
    side = torch.cuda.Stream()
    a = torch.empty(1 << 28, device="cuda", dtype=torch.float32)
    bbuf = torch.empty_like(a)
    bad, ran, skipped = 0, 0, 0
    names = ("gates", "c", "h", "dgates")
    prev = ops.get_compute_dtype()
    try:
        for name, mode, H, T, N, rtol in cases:
            ops.set_compute_dtype(name)
            if not (ops.lstm_persistent_usable(N, H, mode) and ops.lstm_persistent_usable(N, H, mode, bwd=True)):
                log(f"{name} H={H} N={N}: no persistent kernel on this device (skipped)")
                skipped += 1
                continue
            ran += 1
            ref = _pass(mode, H, T, N, False)[:4]                   # (the per-frame launches leave no bias gradient)
            first, case_bad = None, 0
            n_rounds = rounds if T <= 128 else max(1, rounds // 4)      # the long sequences cost 4-8 x per round
            for rnd in range(n_rounds):
                with torch.cuda.stream(side):
                    for _ in range(rnd % 5):
                        bbuf.copy_(a)
                try:
                    got = _pass(mode, H, T, N, True)
                except _lib.DvaeHipError as e:           # a bounded wait gave up: a bad round, not a traceback
                    log(f"MISMATCH {name} H={H} N={N}: round {rnd}: {e}")
                    case_bad += 1
                    continue
                clean = True
                for tn, x, y in zip(names, got, ref):
                    err = (x - y).abs()
                    tol = rtol * float(y.abs().max())
                    wrong = (not bool(torch.isfinite(x).all())) or float(err.max()) > tol
                    if not wrong and first is not None:
                        wrong = not torch.equal(x, first[names.index(tn)])
                    if wrong:
                        e = err.reshape(T, N, -1)
                        frames = (e.amax(dim=(1, 2)) > tol).nonzero().flatten().tolist()
                        rows = (e.amax(dim=(0, 2)) > tol).nonzero().flatten().tolist()
                        log(f"MISMATCH {name} H={H} N={N}: {tn}, round {rnd} ({rnd % 5} GiB of foreign traffic): max |diff| "
                            f"{float(err.max()):.3e} (tolerance {tol:.1e}); frames {frames[:6]}.. ({len(frames)}), rows {rows[:8]}.. ({len(rows)})")
                        case_bad += 1
                        clean = False
                        break
                why = _bias_slabs_wrong(got[4], got[3], T, N, None if first is None else first[4]) if clean else None
                if why:
                    log(f"MISMATCH {name} H={H} N={N}: dbias_part, round {rnd} ({rnd % 5} GiB of foreign traffic): {why}")
                    case_bad += 1
                    clean = False
                if first is None and clean:              # the bitwise reference is a round that matched the frame kernels
                    first = [t.clone() for t in got]
            torch.cuda.synchronize()
            log(f"{name} H={H} N={N} T={T}: {case_bad} bad rounds of {n_rounds}")
            bad += case_bad
    finally:
        ops.set_compute_dtype(prev)      # leave the compute mode as it was found, whatever happened
    try:
        log(f"XCD-local hand-offs (row groups on one XCD, verified per launch): {ops.lstm_pers_local_launches()} launches so far"
            + (" — switched off (DVAE_PERS_XCD_LOCAL=0)" if os.environ.get("DVAE_PERS_XCD_LOCAL", "1")[:1] == "0" else ""))
    except Exception as e:      # statistics only
        log(f"XCD-local statistics unavailable: {e}")
    log(f"selftest cases: {ran} run, {skipped} skipped")
    log("selftest " + ("PASSED" if bad == 0 else f"FAILED: {bad} bad rounds — train on this GPU with DVAE_LSTM_PERSISTENT=0 and report its unique_id"))
    return 0 if bad == 0 else 1


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    torch.cuda.set_device(args.device)
    return run(args.rounds)


if __name__ == "__main__":
    sys.exit(main())
