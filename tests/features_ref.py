"""Host-side helpers of the suites that switch every opt-in feature of the training step on together (gradient clipping with
the non-finite guard, the weight average, the KL schedule with free bits, the speaker adversary, the factor penalty): how a
free-bit threshold is chosen from measured per-dimension KL values, the three device weights of a step restated from DESIGN.md
sections 4.16, 4.18 and 4.19, and the one place that switches everything on.  Not a test module: tests/test_features_ref.py
runs it on the CPU, tests/test_hip_all_features.py uses it on the MI355X.
"""
import numpy as np

# the configuration `all_on` switches on unless told otherwise; the three warm-ups differ on purpose: the three weights
# saturate at different steps
KL = dict(kind="linear", start=1.0, steps=6)
ADV = dict(weight=0.5, hidden=64, warmup_steps=5)
FACTOR = dict(tc_weight=3.0, shared_weight=1.5, warmup_steps=7)
EMA_DECAY = 0.9


def pick_threshold(values):
    """values: the per-dimension KL of one latent group (both halves pooled) -> (lam, margin): the midpoint of the widest gap
    between neighbours of the sorted values whose lower end lies in the middle half of the sorted list (the indices n // 4 ..
    n - n // 4 - 1; the first of several widest gaps), and half that gap.  With lam as the free-bit threshold at least a
    quarter of the values is free and at least a quarter penalised, and no value is nearer to the decision than margin."""
    v = sorted(float(x) for x in values)
    n = len(v)
    if n < 2:
        raise ValueError(f"pick_threshold: {n} value(s), a gap needs two")
    if not all(np.isfinite(x) for x in v):
        raise ValueError("pick_threshold: the values must be finite")
    best = None
    for i in range(n // 4, min(n - n // 4, n - 1)):
        gap = v[i + 1] - v[i]
        if best is None or gap > best[0]:
            best = (gap, i)
    gap, i = best
    return 0.5 * (v[i] + v[i + 1]), 0.5 * gap


def _f32(x):
    return float(np.float32(x))


def _ramp(k, n):
    """min(1, k / n); 1 without a warm-up"""
    return 1.0 if n <= 0 else min(1.0, k / n)


def expected_coefficients(trainer_cfg, k):
    """trainer_cfg: dict(kl_cof=, kl=dict(kind, start, steps) or None, adv=dict(weight, warmup_steps) or None,
    factor=dict(tc_weight, shared_weight, warmup_steps) or None) as `all_on` returns it; k: the number of optimiser steps taken
    before the step.  -> (KL weight, adversary weight, (w_tc, w_sh)) as the float32 values the device holds, None for a
    feature that is off.  DESIGN.md 4.16: constant kl_cof; linear start + (kl_cof - start) k / steps below steps, kl_cof from
    there on.  4.18: weight min(1, k / warmup_steps).  4.19: (tc_weight, shared_weight) min(1, k / warmup_steps)."""
    k = int(k)
    kl = adv = fac = None
    if trainer_cfg.get("kl") is not None:
        c, top = trainer_cfg["kl"], float(trainer_cfg["kl_cof"])
        if c["kind"] == "constant":
            kl = top
        elif c["kind"] == "linear":
            kl = top if k >= c["steps"] else c["start"] + (top - c["start"]) * (k / c["steps"])
        else:
            raise ValueError(f"expected_coefficients: no restatement of the {c['kind']!r} schedule")
        kl = _f32(kl)
    if trainer_cfg.get("adv") is not None:
        c = trainer_cfg["adv"]
        adv = _f32(c["weight"] * _ramp(k, c["warmup_steps"]))
    if trainer_cfg.get("factor") is not None:
        c = trainer_cfg["factor"]
        f = _ramp(k, c["warmup_steps"])
        fac = (_f32(c["tc_weight"] * f), _f32(c["shared_weight"] * f))
    return kl, adv, fac


def all_on(w, *, spk, max_norm, free_bits, kl=KL, adv=ADV, factor=FACTOR, ema=EMA_DECAY):
    """Switch every opt-in feature on for a trainer from kernel_harness.make_trainer: the KL schedule `kl` with `free_bits`
    (None, or a (style, content) pair), the adversary `adv` on `spk` speakers, the factor penalty `factor`, set_grad_clip(max_norm)
    and set_ema(ema).  None for `kl`, `adv`, `factor`, `max_norm` or `ema` leaves that one off.  -> the configuration
    `expected_coefficients` takes."""
    cfg = dict(kl_cof=float(w.kl_cof), kl=None, adv=None, factor=None)
    if kl is not None:
        w.set_kl_schedule(kl["kind"], start=kl.get("start", 0.0), steps=kl.get("steps", 0), free_bits=free_bits)
        cfg["kl"] = dict(kl)
    if adv is not None:
        w.set_speaker_adversary(adv["weight"], n_speakers=spk, hidden=adv["hidden"], warmup_steps=adv["warmup_steps"])
        cfg["adv"] = dict(adv)
    if factor is not None:
        w.set_factor_penalty(factor["tc_weight"], factor["shared_weight"], warmup_steps=factor["warmup_steps"])
        cfg["factor"] = dict(factor)
    if max_norm is not None:
        w.optimizer.set_grad_clip(max_norm)
    if ema is not None:
        w.optimizer.set_ema(ema)
    return cfg
