"""tests/kl_sched_ref.py on the CPU: the restated backward is the gradient of the restated forward, the fp32 statement of the
kernel stays inside the derived bounds, the free-bits inputs of every GPU shape keep their margin from the gate, and the
schedule (dvae_amd.kl_schedule) is the pure function of the step count the trainer takes it for."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import elem_ref as E  # noqa: E402
import kl_sched_ref as R  # noqa: E402
from ref_common import worst_ratio  # noqa: E402

F32, F64 = np.float32, np.float64


def _cases():
    return [(rows, D, single) for rows, D in R.SHAPES for single in (("free", "on") if D == 1 else ("free",))]


# ------------------------------------------------------------------ the inputs of the GPU tests
@pytest.mark.parametrize("rows,D,single", _cases())
def test_free_bits_inputs_keep_their_margin(rows, D, single):
    for n in R.NS:
        d = R.inputs(rows, D, n, 1000 + rows + D)
        lam = R.free_bits_for(d, single)                    # asserts the margin and both classes itself
        R.check_margin(d, lam)
        _, aux = R.fwd(d, (10.0, 3.0), lam)
        gate = aux[4 + 2 * D:].reshape(2, D)
        assert aux[2] == D - gate[0].sum() and aux[3] == D - gate[1].sum()
        if D > 1:
            assert 0 < aux[2] < D and 0 < aux[3] < D
        else:
            assert aux[2] == aux[3] == (1.0 if single == "free" else 0.0)
        assert (lam >= 0).all()


@pytest.mark.parametrize("rows,D", R.SHAPES)
def test_positive_inputs_gate_everything_on(rows, D):
    d = R.positive_inputs(rows, D, 4, 2000 + rows + D)
    lam = np.zeros(D, F32)
    R.check_margin(d, lam)
    _, aux = R.fwd(d, (10.0, 3.0), lam)
    assert (aux[4 + 2 * D:] == 1.0).all() and aux[2] == aux[3] == 0.0
    assert (R.kl_dim(d) > 0).all()


def test_bit_cases_divide():
    for n, nq, ns in R.bit_cases():
        ds = R.divisors(nq)
        assert ds and all(nq % D == 0 and 1 <= D <= R.LOSS_MAX_D for D in ds)
    assert R.divisors(255) == [1, 5, 255] and R.divisors(257) == [1, 257] and R.divisors(1) == [1]
    # what the shapes reach: one row, one column, more columns than one pass of 256 threads, more rows than threads, the cap
    assert any(r == 1 for r, _ in R.SHAPES) and any(D == 1 for _, D in R.SHAPES)
    assert any(D > 256 and D % 256 for _, D in R.SHAPES) and any(r > 256 for r, _ in R.SHAPES)
    assert any(D == R.LOSS_MAX_D for _, D in R.SHAPES)
    hdr = open(os.path.join(ROOT, "include", "dvae_hip.h")).read()
    assert int(re.search(r"#define DVAE_LOSS_MAX_D (\d+)", hdr).group(1)) == R.LOSS_MAX_D


# ------------------------------------------------------------------ the restatement
def test_without_free_bits_it_is_elem_ref():
    d = R.inputs(3, 5, 1023, 5)
    out, aux = R.fwd(d, (10.0, 3.0))
    ref = E.loss_fwd(dict(d, mse_cof=F32(10.0), kl_cof=F32(3.0)))
    assert np.array_equal(out[1:], ref[1:]) and abs(out[0] - ref[0]) <= 1e-12 * abs(ref[0])
    assert np.array_equal(aux[:2], ref[5:7]) and (aux[2:4] == 0).all() and (aux[4 + 10:] == 1).all()
    # the per-dimension means add up to the term
    assert np.allclose(aux[4:4 + 10].reshape(2, 5).sum(1), ref[5:7], rtol=1e-13, atol=0)
    for gname, g8 in E.G8.items():
        a, b = R.bwd(d, (10.0, 3.0), g8.astype(F64)), E.loss_bwd(dict(d, mse_cof=F32(10.0), kl_cof=F32(3.0)), g8.astype(F64))
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), gname


def test_free_bits_forward_by_hand():
    d = R.inputs(2, 2, 4, 7)
    for k, v in (("q1_mu", [1.0, 0.0, 1.0, 0.0]), ("q1_lv", [0.0, 0.0, 0.0, 0.0]), ("q2_mu", [0.0, 2.0, 0.0, 2.0]),
                 ("q2_lv", [0.0, 0.0, 0.0, 0.0])):
        d[k] = np.asarray(v, F32)
    # KL per element = mu^2 / 2 at lv = 0: kl_dim z1 = (0.5, 0), z2 = (0, 2)
    assert np.allclose(R.kl_dim(d), [[0.5, 0.0], [0.0, 2.0]], atol=1e-15)
    out, aux = R.fwd(d, (0.0, 1.0), np.asarray([0.25, 0.25], F32))
    assert np.allclose(aux[:4], [0.75, 2.25, 1.0, 1.0]) and np.allclose(aux[8:], [1, 0, 0, 1])
    assert np.isclose(out[0], 3.0) and np.isclose(out[5], 0.5) and np.isclose(out[6], 2.0)       # raw terms stay raw
    # strict: a dimension exactly at lambda is free
    _, aux = R.fwd(d, (0.0, 1.0), np.asarray([0.5, 2.0], F32))
    assert list(aux[8:]) == [0, 0, 0, 0] and list(aux[2:4]) == [2, 2] and np.allclose(aux[:2], [2.5, 2.5])


@pytest.mark.parametrize("rows,D", [(1, 1), (3, 5), (4, 32)])
def test_backward_is_the_gradient_of_forward(rows, D):
    """Central differences in float64 on every latent statistic, away from the gate (the inputs keep their margin)."""
    d = R.inputs(rows, D, 4, 31 + rows)
    lam = R.free_bits_for(d)
    coef, g8 = (10.0, 3.0), E.G8["random"].astype(F64)
    _, aux = R.fwd(d, coef, lam)
    gate = aux[4 + 2 * D:].reshape(2, D)
    grads = R.bwd(d, coef, g8, gate)
    d64 = {k: (np.asarray(v, F64) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    f = lambda dd: float(np.dot(g8, R.fwd(dd, coef, lam)[0]))
    h = 1e-6
    for key, j in (("q1_mu", 4), ("q1_lv", 5), ("q2_mu", 6), ("q2_lv", 7), ("s_mu", 8), ("s_lv", 9)):
        for i in range(min(d64[key].size, 12)):
            up, dn = dict(d64), dict(d64)
            up[key], dn[key] = d64[key].copy(), d64[key].copy()
            up[key][i] += h
            dn[key][i] -= h
            num = (f(up) - f(dn)) / (2 * h)
            assert abs(num - grads[j][i]) <= 1e-6 * max(1.0, abs(grads[j][i])), (key, i, num, grads[j][i])


def test_free_dimensions_take_nothing_from_the_total():
    d = R.inputs(4, 32, 4, 9)
    lam = R.free_bits_for(d)
    _, aux = R.fwd(d, (10.0, 3.0), lam)
    gate = aux[4 + 64:].reshape(2, 32)
    grads = R.bwd(d, (10.0, 3.0), E.G8["total"].astype(F64), gate)
    for k in range(2):
        free = np.tile(gate[k] == 0, 4)
        assert (grads[4 + 2 * k][free] == 0).all() and (grads[5 + 2 * k][free] == 0).all()
        assert (grads[4 + 2 * k][~free] != 0).any()
    # ... and keep the direct gradient of out8[5 + k]
    g = np.zeros(8)
    g[5], g[6] = 1.0, -2.0
    a, b = R.bwd(d, (10.0, 3.0), g, gate), R.bwd(d, (10.0, 3.0), g, None)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("rows,D,single", _cases())
def test_fp32_statement_is_inside_the_bounds(rows, D, single):
    """kl_dim and the clamped sums as the kernel states them, with an expf pushed to either end of its bound."""
    d = R.inputs(rows, D, 4, 1000 + rows + D)
    lam = R.free_bits_for(d, single)
    out, aux, tol8, taux = R.fwd_bounds(d, (10.0, 3.0), lam)
    for push in (-1, 0, 1):
        kd, gate, a = R.fwd_f32(d, (10.0, 3.0), lam, push)
        r, i = worst_ratio(kd.reshape(-1).astype(F64), aux[4:4 + 2 * D], taux[4:4 + 2 * D])
        assert r <= 1.0, (push, i, r)
        assert np.array_equal(gate.reshape(-1).astype(F64), aux[4 + 2 * D:])
        r, i = worst_ratio(a.astype(F64), aux[:2], taux[:2])
        assert r <= 1.0, (push, i, r)
    # the margin is what the gate's exactness rests on: ten bounds and more on every column
    assert (np.abs(aux[4:4 + 2 * D].reshape(2, D) - lam.astype(F64)[None]) >= R.MARGIN * taux[4:4 + 2 * D].reshape(2, D)).all()


# ------------------------------------------------------------------ the schedule
def _sched(*a, **k):
    from dvae_amd.kl_schedule import KLSchedule
    return KLSchedule(*a, **k)


def test_constant_and_linear():
    assert [_sched("constant").weight_at(k, 1, 10.0) for k in (0, 5, 10 ** 6)] == [10.0] * 3
    s = _sched("linear", start=0.0, steps=5)
    w = [s.weight_at(k, 1, 10.0) for k in range(9)]
    assert w[0] == 0.0 and w[5:] == [10.0] * 4 and w[:6] == [0.0, 2.0, 4.0, 6.0, 8.0, 10.0]
    s = _sched("linear", start=0.5, steps=7)
    w = [s.weight_at(k, 3, 4.0) for k in range(12)]
    assert w[0] == 0.5 and w[7] == 4.0 and all(b >= a for a, b in zip(w, w[1:])) and max(w) == 4.0
    # downwards too: a start above the target
    w = [_sched("linear", start=20.0, steps=4).weight_at(k, 1, 10.0) for k in range(6)]
    assert w == [20.0, 17.5, 15.0, 12.5, 10.0, 10.0]


def test_cyclical_boundaries():
    s = _sched("cyclical", start=0.0, steps=40, cycles=4, ratio=0.5)
    w = [s.weight_at(k, 1, 10.0) for k in range(45)]
    for c in range(4):
        assert w[10 * c] == 0.0                                 # every cycle starts from `start`
        assert w[10 * c + 5:10 * c + 10] == [10.0] * 5          # holds from ratio x cycle on
        ramp = w[10 * c:10 * c + 6]
        assert ramp == [0.0, 2.0, 4.0, 6.0, 8.0, 10.0]
    assert w[40:] == [10.0] * 5                                 # after `steps`: kl_cof
    # a cycle of a fractional number of steps: positions in integers, still start at every boundary that is a step
    s = _sched("cyclical", start=1.0, steps=10, cycles=4, ratio=1.0)
    w = [s.weight_at(k, 1, 3.0) for k in range(12)]
    assert w[0] == 1.0 and w[5] == 1.0 and w[10:] == [3.0, 3.0] and all(1.0 <= v < 3.0 for v in w[:10])
    assert _sched("cyclical", steps=8, cycles=1, ratio=0.5).weight_at(4, 1, 10.0) == 10.0


def test_double_is_the_reference_update_kl():
    for start, cap in ((0.01, 10.0), (1.0, 10.0), (3.0, 10.0), (10.0, 10.0), (0.3, 7.0)):
        s, kl, seq = _sched("double", start=start), start, []
        for epoch in range(1, 16):
            seq.append(kl)
            kl = min(kl * 2, cap)           # update_kl(), once per epoch (cap 10 in the reference)
        got = [s.weight_at(123, e, cap) for e in range(1, 16)]
        assert got == [min(v, cap) for v in seq]
        assert all(b >= a for a, b in zip(got, got[1:])) and got[-1] == cap
    assert _sched("double", start=1.0).weight_at(0, 5000, 10.0) == 10.0


def test_resume_continues_the_uninterrupted_run():
    for kw in (dict(kind="linear", start=0.1, steps=17), dict(kind="cyclical", start=0.0, steps=23, cycles=3, ratio=0.4),
               dict(kind="double", start=0.5), dict(kind="constant")):
        a = _sched(**kw)
        whole = [a.weight_at(k, 1 + k // 6, 10.0) for k in range(40)]
        b = _sched(**a.params())                    # what a checkpoint keeps is enough to build it again
        assert b.params() == a.params()
        k0 = 11                                     # ... and the position is the step count
        assert [b.weight_at(k, 1 + k // 6, 10.0) for k in range(k0, 40)] == whole[k0:]


def test_argument_errors():
    from dvae_amd.kl_schedule import expand_free_bits
    for bad in (dict(kind="cosine"), dict(kind="linear", steps=0), dict(kind="linear", steps=-1), dict(kind="linear", steps=2.5),
                dict(kind="linear", steps=5, start=-1.0), dict(kind="linear", steps=5, start=float("nan")),
                dict(kind="cyclical", steps=4, cycles=0), dict(kind="cyclical", steps=4, cycles=5),
                dict(kind="cyclical", steps=4, ratio=0.0), dict(kind="cyclical", steps=4, ratio=1.5), dict(kind="double", start=0.0)):
        with pytest.raises(ValueError):
            _sched(**bad)
    with pytest.raises(ValueError):
        _sched("constant").weight_at(-1)
    with pytest.raises(ValueError):
        _sched("constant").weight_at(0, 0)
    assert expand_free_bits(None, 4, 28) is None
    assert expand_free_bits(0.5, 1, 2) == [0.5] * 3
    assert expand_free_bits((0.0, 0.05), 4, 28) == [0.0] * 4 + [0.05] * 28
    assert expand_free_bits(list(range(32)), 4, 28) == [float(v) for v in range(32)]
    for bad in ((1.0, 2.0, 3.0), -0.1, (0.1, float("inf")), [0.0] * 31):
        with pytest.raises(ValueError):
            expand_free_bits(bad, 4, 28)


# ------------------------------------------------------------------ plumbing
def test_header_and_binding_agree():
    from dvae_amd import _lib
    import __graft_entry__ as ge
    decl = ge.declared_symbols()
    for name in ("dvae_loss_fwd_sched", "dvae_loss_bwd_sched"):
        assert name in decl and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["dvae_loss_fwd_sched"][1]) == 6 and len(_lib.SIGNATURES["dvae_loss_bwd_sched"][1]) == 15
    assert [f[0] for f in _lib.LossSched._fields_] == ["coef", "free_bits", "D"]
    assert _lib.LOSS_MAX_D == R.LOSS_MAX_D
    # the two legacy calls keep their argument lists
    assert len(_lib.SIGNATURES["dvae_loss_fwd"][1]) == 4 and len(_lib.SIGNATURES["dvae_loss_bwd"][1]) == 13


def test_cli_flags():
    from dvae_amd.train import get_parse, kl_schedule_args
    p = get_parse()
    assert kl_schedule_args(p.parse_args([]))[0] is None
    kind, kw = kl_schedule_args(p.parse_args(["--free-bits-content", "0.05"]))
    assert kind == "constant" and kw["free_bits"] == (0.0, 0.05)
    kind, kw = kl_schedule_args(p.parse_args(["--kl-schedule", "cyclical", "--kl-warmup-steps", "40", "--kl-cycles", "2",
                                              "--kl-ratio", "0.25", "--kl-start", "0.5", "--free-bits", "0.1",
                                              "--free-bits-style", "0.2"]))
    assert kind == "cyclical" and kw == dict(start=0.5, steps=40, cycles=2, ratio=0.25, free_bits=(0.2, 0.1))
    a = p.parse_args(["--style_cof", "0.3", "--beta_cof", "0.2"])           # still parsed, still unused
    assert a.style_cof == 0.3 and a.beta_cof == 0.2
