"""The float64 restatement of the smoothing penalty (tests/msloss_ref.py) on the CPU: its closed-form
gradient against torch's float64 autograd and central differences, its figures against the over-smoothing instruments'
restatement (section 4.14) with the floor taken away, what it says about a smoothed and about a constant trajectory, the
mutations the device comparison must be able to tell from the statement, and the plumbing (header, binding)."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import modspec_ref as MR  # noqa: E402
import msloss_ref as R  # noqa: E402
from ref_common import F64, worst_ratio  # noqa: E402


def case(seed, Bh, C, T):
    rs = np.random.RandomState(seed)
    x = rs.uniform(0.0, 1.0, (2 * Bh, C, T))
    y = np.clip(x + 0.2 * rs.randn(*x.shape), 0.0, 1.0)
    return y, x[:Bh], x[Bh:]


def torch_loss(y, x1, x2, D, floor, w_ms, w_gv):
    """the definitions once more, in torch float64 with an FFT: independent of the restatement's table and closed forms"""
    x = torch.cat([x1, x2], 0)
    N, C, T = y.shape

    def figures(a):
        w = a.reshape(N, C, T // D, D)
        d = w - w.mean(-1, keepdim=True)
        Y = torch.fft.rfft(d, dim=-1)[..., 1:]
        s = torch.log(Y.real ** 2 + Y.imag ** 2 + D * floor * floor)
        v = ((a - a.mean(-1, keepdim=True)) ** 2).mean(-1)
        return s, torch.log(v + floor * floor)
    (s, g), (sx, gx) = figures(y), figures(x)
    return w_ms * ((s - sx) ** 2).mean() + w_gv * ((g - gx) ** 2).mean()


@pytest.mark.parametrize("Bh,C,T,D", [(1, 2, 16, 8), (2, 3, 48, 24), (1, 5, 64, 64)])
def test_closed_form_gradient_against_autograd_and_differences(Bh, C, T, D):
    y, x1, x2 = case(Bh + C + T, Bh, C, T)
    w_ms, w_gv, floor = 0.7, 1.3, 0.003
    r = R.evaluate(y, x1, x2, D, floor, w_ms, w_gv)
    ty = torch.tensor(y, dtype=torch.float64, requires_grad=True)
    loss = torch_loss(ty, torch.tensor(x1), torch.tensor(x2), D, floor, w_ms, w_gv)
    assert math.isclose(loss.item(), r["stats"][4], rel_tol=1e-12)
    loss.backward()
    g = ty.grad.numpy()
    assert np.abs(r["dy"] - g).max() <= 1e-12 * np.abs(g).max()
    rs = np.random.RandomState(0)
    for _ in range(6):
        i = tuple(rs.randint(0, n) for n in y.shape)
        h = 1e-6
        yp, ym = y.copy(), y.copy()
        yp[i] += h
        ym[i] -= h
        num = (R.loss(yp, x1, x2, D, floor, w_ms, w_gv) - R.loss(ym, x1, x2, D, floor, w_ms, w_gv)) / (2 * h)
        assert math.isclose(num, r["dy"][i], rel_tol=1e-5, abs_tol=1e-9 * np.abs(g).max()), (i, num, r["dy"][i])
    # the incoming gradient scales it
    assert np.array_equal(R.evaluate(y, x1, x2, D, floor, w_ms, w_gv, gscale=2.0)["dy"], 2.0 * r["dy"])


def test_without_the_floor_the_figures_are_section_4_14s():
    y, x1, x2 = case(5, 2, 4, 32)
    y = y.astype(np.float32)
    D = 16
    r = R.evaluate(y, x1, x2, D, floor=1e-150)
    N, C, T = y.shape
    windows = y.reshape(N, C, T // D, D)
    m = MR.modspec(windows)
    assert np.allclose(r["a"]["s"], m["s"], rtol=1e-10, atol=1e-10)
    packed = np.ascontiguousarray(y.transpose(1, 0, 2).reshape(C, N * T))
    gv = MR.gv(packed, [(n * T, T, 0, 0) for n in range(N)])
    assert np.allclose(r["a"]["g"], np.log(gv["v"]), rtol=1e-12) and np.allclose(r["a"]["m"], gv["m"], rtol=1e-12)
    # and the two reported figures are its distance and its ratio
    x = np.concatenate([x1, x2], 0)
    sx = MR.modspec(x.astype(np.float32).reshape(N, C, T // D, D))["s"]
    rx = R.evaluate(y, x1.astype(np.float32), x2.astype(np.float32), D, floor=1e-150)
    assert math.isclose(rx["stats"][2], MR.DB * math.sqrt(((m["s"] - sx) ** 2).mean()), rel_tol=1e-9)


def test_a_smoothed_target_is_smoother_and_the_gradient_repairs_it():
    rs = np.random.RandomState(3)
    x = rs.uniform(0.0, 1.0, (4, 6, 64))
    y = sum(np.roll(x, k, -1) for k in (-2, -1, 0, 1, 2)) / 5.0
    x1, x2 = x[:2], x[2:]
    r = R.evaluate(y, x1, x2, 32, 0.003, 1.0, 1.0)
    assert r["stats"][3] < 0 and r["stats"][2] > 0
    ms, gv = [r["stats"][0]], [r["stats"][1]]
    for _ in range(5):
        y = y - 0.01 * R.evaluate(y, x1, x2, 32, 0.003, 1.0, 1.0)["dy"] / np.abs(r["dy"]).max()
        s = R.evaluate(y, x1, x2, 32, 0.003, 1.0, 1.0)["stats"]
        ms.append(s[0])
        gv.append(s[1])
    assert all(b < a for a, b in zip(ms, ms[1:])) and all(b < a for a, b in zip(gv, gv[1:])), (ms, gv)


def test_a_constant_trajectory_is_finite_with_a_zero_gradient():
    _, x1, x2 = case(1, 1, 3, 16)
    y = np.full((2, 3, 16), 0.5)
    r = R.evaluate(y, x1, x2, 8)
    assert np.isfinite(r["stats"]).all() and np.isfinite(r["dy"]).all() and not r["dy"].any()
    sb, db = R.bounds(r)
    assert np.isfinite(sb).all() and np.isfinite(db).all()
    # |ds / dd_t| <= 1 / sqrt(eps_ms): the stabiliser bounds the gradient of every element
    y2, x1, x2 = case(2, 1, 3, 16)
    a = R.evaluate(y2, x1, x2, 8)["a"]
    assert (2.0 * np.sqrt(a["P"]) / (a["P"] + a["eps_ms"]) <= 1.0 / math.sqrt(a["eps_ms"]) * (1 + 1e-12)).all()


@pytest.mark.parametrize("Bh,C,T,D", R.SHAPES)
def test_bounds_are_tight_and_mutations_exceed_them(Bh, C, T, D):
    """on the GPU suite's own inputs: the bounds are a few fp32 roundings wide, and every mutation of the statement leaves them"""
    c = R.kernel_case(Bh, C, T, D)
    r = R.evaluate(c["y"], c["x1"], c["x2"], D)
    sb, db = R.bounds(r)
    assert np.isfinite(sb).all() and np.isfinite(db).all() and (sb > 0).all() and (db > 0).all()
    assert (sb <= 4 * 2.0 ** -24 * np.abs(r["stats"]) + 1e-30).all()
    assert (db <= 2.0 ** -24 * np.abs(r["dy"]) + 1e-9 * np.abs(r["dy"]).max() + 1e-30).all()
    assert not r["dy"][0, C - 1].any() and r["dy"].any()                     # the constant bin; not everything
    # the restatement rounded to fp32 stays inside its own bounds
    assert worst_ratio(r["stats"].astype(np.float32), r["stats"], sb)[0] <= 1.0
    assert worst_ratio(r["dy"].astype(np.float32), r["dy"], db)[0] <= 1.0
    for mut in R.MUTATIONS:
        if mut == "var_div_D" and T == D:      # one window a row: the two divisors are one number
            continue
        m = R.evaluate(c["y"], c["x1"], c["x2"], D, mut=mut)
        worst = max(worst_ratio(m["stats"], r["stats"], sb)[0], worst_ratio(m["dy"], r["dy"], db)[0])
        assert worst > 1.0, (mut, worst)
    assert set(R.MUTATIONS) == {"k0", "no_centring", "im_sign", "var_div_D", "sum_for_mean", "eps_without_D", "halves_swapped"}
    assert any(t != d for _, _, t, d in R.SHAPES)                            # var_div_D is told apart somewhere


def test_refused_arguments():
    y, x1, x2 = case(1, 1, 2, 16)
    for D in (7, 6, 12, 130):
        with pytest.raises(ValueError):
            R.evaluate(y, x1, x2, D)
    with pytest.raises(ValueError):
        R.evaluate(y, x1, x2, 8, floor=0.0)
    assert R.default_window(128) == 64 and R.default_window(24) == 24


def test_header_and_binding_declare_the_entry_points():
    from dvae_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dvae_hip.h")).read()
    for name in ("dvae_msloss_ws_bytes", "dvae_msloss_fwd", "dvae_msloss_bwd"):
        assert re.search(r"\b" + name + r"\(", hdr) and name in _lib.SIGNATURES
    n_args = lambda name: len(re.search(name + r"\(([^;]*)\);", hdr).group(1).split(","))
    for name in ("dvae_msloss_ws_bytes", "dvae_msloss_fwd", "dvae_msloss_bwd"):
        assert n_args(name) == len(_lib.SIGNATURES[name][1]), name
    assert int(re.search(r"#define DVAE_ABI_VERSION (\d+)", hdr).group(1)) == 319
    assert int(re.search(r"#define DVAE_MODSPEC_DMIN (\d+)", hdr).group(1)) == R.D_MIN
    assert int(re.search(r"#define DVAE_MODSPEC_DMAX (\d+)", hdr).group(1)) == R.D_MAX
