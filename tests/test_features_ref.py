"""tests/features_ref.py on the CPU: the threshold chooser on hand-made lists, the three device weights against hand values
(exact fractions rounded to float32), and what `all_on` asks of a trainer."""
from fractions import Fraction

import numpy as np
import pytest

import features_ref as F


# ------------------------------------------------------------------ pick_threshold
def test_threshold_is_the_midpoint_of_the_widest_gap_in_the_middle_half():
    # eight values: the lower ends with sorted index 2 .. 5 count; the gaps 0 -> 1 (0.9) and 6 -> 7 (5) lie outside
    vals = [0.0, 0.9, 1.0, 1.1, 1.5, 1.6, 1.9, 7.0]
    lam, margin = F.pick_threshold(vals)
    assert lam == 0.5 * (1.1 + 1.5) and margin == 0.5 * (1.5 - 1.1)
    # the order of the input is irrelevant
    assert F.pick_threshold(list(reversed(vals))) == (lam, margin)
    assert F.pick_threshold(np.array(vals)[[3, 7, 1, 0, 6, 2, 5, 4]]) == (lam, margin)
    # the gap whose lower end is the last index of the middle half (5 -> 6) counts
    lam, margin = F.pick_threshold([0.0, 0.9, 1.0, 1.1, 1.2, 1.3, 2.0, 7.0])
    assert lam == 0.5 * (1.3 + 2.0) and margin == 0.5 * (2.0 - 1.3)
    # some values lie on either side: a threshold that frees some dimensions and penalises others
    assert sum(v <= lam for v in vals) >= 2 and sum(v > lam for v in vals) >= 2


def test_threshold_with_ties():
    # the model's style dimensions: both halves hold the same posterior, every value comes twice
    lam, margin = F.pick_threshold([1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 4.5, 4.5])
    assert (lam, margin) == (3.0, 1.0)
    # two gaps of one width: the lower one
    assert F.pick_threshold([0.0, 0.0, 1.0, 2.0, 3.0, 3.0, 3.0, 9.0])[0] == 1.5
    # every value the same: the midpoint is the value and the margin is 0 (the caller's condition on the margin refuses it)
    assert F.pick_threshold([0.25] * 6) == (0.25, 0.0)


def test_threshold_of_two_values_and_refusals():
    assert F.pick_threshold([3.0, 1.0]) == (2.0, 1.0)
    assert F.pick_threshold([1.0, 2.0, 4.0]) == (3.0, 1.0)
    for bad in ([], [1.0], [1.0, float("nan")], [1.0, float("inf")]):
        with pytest.raises(ValueError):
            F.pick_threshold(bad)


# ------------------------------------------------------------------ expected_coefficients
CFG = dict(kl_cof=10.0, kl=dict(kind="linear", start=1.0, steps=6), adv=dict(weight=0.5, hidden=64, warmup_steps=5),
           factor=dict(tc_weight=3.0, shared_weight=1.5, warmup_steps=7))


def is_f32_of(v, frac):
    """v is a float32 value and the nearest one to the exact fraction"""
    if v != float(np.float32(v)):
        return False
    if frac == 0:
        return v == 0.0
    e = 0
    while Fraction(2) ** e > abs(frac):
        e -= 1
    while Fraction(2) ** (e + 1) <= abs(frac):
        e += 1
    return abs(Fraction(v) - frac) <= Fraction(2) ** (e - 24)


def test_is_f32_of_is_strict_enough():
    assert is_f32_of(float(np.float32(0.3)), Fraction(3, 10)) and not is_f32_of(0.3, Fraction(3, 10))
    assert not is_f32_of(float(np.nextafter(np.float32(0.3), np.float32(1))), Fraction(3, 10))
    assert is_f32_of(5.5, Fraction(11, 2)) and not is_f32_of(5.5, Fraction(11, 2) + Fraction(1, 1000))


def test_linear_ramp_hand_values():
    got = [F.expected_coefficients(CFG, k)[0] for k in (0, 3, 6, 9)]
    assert got == [1.0, 5.5, 10.0, 10.0]
    assert [F.expected_coefficients(CFG, k)[0] for k in (1, 2, 4, 5)] == [2.5, 4.0, 7.0, 8.5]
    const = dict(CFG, kl=dict(kind="constant"))
    assert [F.expected_coefficients(const, k)[0] for k in (0, 4, 100)] == [10.0] * 3


def test_adversary_hand_values():
    got = [F.expected_coefficients(CFG, k)[1] for k in (0, 3, 6, 9)]
    assert got[0] == 0.0 and got[2:] == [0.5, 0.5] and is_f32_of(got[1], Fraction(3, 10))
    for k in range(1, 5):
        assert is_f32_of(F.expected_coefficients(CFG, k)[1], Fraction(k, 10)), k
    assert F.expected_coefficients(CFG, 5)[1] == 0.5
    now = dict(CFG, adv=dict(weight=0.5, hidden=64, warmup_steps=0))
    assert F.expected_coefficients(now, 0)[1] == 0.5


def test_factor_hand_values():
    got = [F.expected_coefficients(CFG, k)[2] for k in (0, 3, 6, 9)]
    assert got[0] == (0.0, 0.0) and got[3] == (3.0, 1.5)
    assert is_f32_of(got[1][0], Fraction(9, 7)) and is_f32_of(got[1][1], Fraction(9, 14))
    assert is_f32_of(got[2][0], Fraction(18, 7)) and is_f32_of(got[2][1], Fraction(9, 7))
    assert F.expected_coefficients(CFG, 7)[2] == (3.0, 1.5)
    now = dict(CFG, factor=dict(tc_weight=40.0, shared_weight=25.0, warmup_steps=0))
    assert F.expected_coefficients(now, 0)[2] == (40.0, 25.0)


def test_the_three_counters_saturate_at_different_steps():
    full = (10.0, 0.5, (3.0, 1.5))
    first = [next(k for k in range(20) if F.expected_coefficients(CFG, k)[i] == full[i]) for i in range(3)]
    assert first == [6, 5, 7]
    assert F.expected_coefficients(dict(kl_cof=10.0), 3) == (None, None, None)
    with pytest.raises(ValueError):
        F.expected_coefficients(dict(CFG, kl=dict(kind="cyclical", start=0.0, steps=4)), 1)


# ------------------------------------------------------------------ all_on
class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a, **kw: self.calls.append((name, a, kw))


def test_all_on_asks_for_the_documented_configuration():
    w = _Recorder()
    w.kl_cof, w.optimizer = 10, _Recorder()
    cfg = F.all_on(w, spk=3, max_norm=12.5, free_bits=(0.1, 0.2))
    assert w.calls == [("set_kl_schedule", ("linear",), dict(start=1.0, steps=6, free_bits=(0.1, 0.2))),
                       ("set_speaker_adversary", (0.5,), dict(n_speakers=3, hidden=64, warmup_steps=5)),
                       ("set_factor_penalty", (3.0, 1.5), dict(warmup_steps=7))]
    assert w.optimizer.calls == [("set_grad_clip", (12.5,), {}), ("set_ema", (0.9,), {})]
    assert cfg == CFG
    # what is None stays off, and the configuration says so
    w = _Recorder()
    w.kl_cof, w.optimizer = 10, _Recorder()
    cfg = F.all_on(w, spk=3, max_norm=None, free_bits=None, adv=None, ema=None,
                   factor=dict(tc_weight=0.0, shared_weight=0.0, warmup_steps=0), kl=dict(kind="constant"))
    assert [c[0] for c in w.calls] == ["set_kl_schedule", "set_factor_penalty"] and w.optimizer.calls == []
    assert w.calls[0] == ("set_kl_schedule", ("constant",), dict(start=0.0, steps=0, free_bits=None))
    assert F.expected_coefficients(cfg, 4) == (10.0, None, (0.0, 0.0))
