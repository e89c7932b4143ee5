"""The float64 reference of the LSTM recurrence kernels (tests/lstm_ref.py), proved without a GPU.

1. Free-running, `lstm_ref` against torch.nn.LSTM in float64 with autograd: h, c, the gate gradients (the dX side of an
   identity input projection) and the bias gradients as their column sums, one direction, the reverse one and both, at
   H = 8 and 64, T = 6, to 1e-12 of each element: pins the gate order, the reverse direction and the cell-gradient carry.
2. The bounds of tests/lstm_ref.py on a numpy float32 restatement of the kernels' statements (sequential fp32 products,
   the gate functions written as in csrc/common.h, epilogues with and without fused multiply-add) on every unit class of
   `make_entry`: error / bound <= 1 for every quantity — the derivation is checked before a GPU is asked.
3. Mutations: each way a kernel could be wrong that the GPU test is there for must be flagged (ratio > 1).
4. Every case of `CASES` selects the kernel its note names: the dispatch arithmetic of csrc/lstm.hip (plan_seq, the H = 64
   rows rule) and csrc/lstm_pers.hip (pers_mt, pers_x3_ok, the 16-row / 8-unit / k-split rules) restated here.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_ref as R  # noqa: E402

F, F64 = np.float32, np.float64


def _relclose(a, b, what, rel=1e-12):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    bad = np.abs(a - b) > rel * np.abs(b) + 1e-300
    assert a.shape == b.shape and not bad.any(), (what, int(bad.sum()), a[bad][:3], b[bad][:3])


def _worst(res):
    return max(r for r, _ in res.values())


# ------------------------------------------------------------------ 1. against torch.nn.LSTM in float64
@pytest.mark.parametrize("H", [8, 64])
@pytest.mark.parametrize("dirs", ["forward", "reverse", "both"])
def test_free_running_reference_matches_torch_lstm_float64(H, dirs):
    T, N = 6, 3
    rs = np.random.RandomState(H + len(dirs))
    # No sum of this data cancels (g, W, dh > 0, hence c, h, dc and every gate gradient > 0): float64 itself does not hold a
    # cancelling sum to 1e-12 of its RESULT, and two float64 programs that add in different orders then differ by more.
    # Nor does a gate saturate (|pre-activation| < 1, c < 2): 1 - g^2 and 1 - tanh^2 c amplify the last bit of two tanh routines.
    x = [rs.uniform(-0.5, 0.5, (T, N, 4 * H)) for _ in range(2)]        # pre-activations per direction
    for xd in x:
        xd[:, :, 2 * H:3 * H] = rs.uniform(0.1, 0.5, (T, N, H))
    W = [rs.uniform(0, 1, (4 * H, H)) / H for _ in range(2)]
    dh = [rs.uniform(0.1, 1, (T, N, H)) for _ in range(2)]
    use = {"forward": (0,), "reverse": (1,), "both": (0, 1)}[dirs]
    # the input is both directions' pre-activations side by side, W_ih picks each direction's own block, biases zero
    lstm = torch.nn.LSTM(8 * H, H, bidirectional=True).double()
    eye = np.eye(4 * H)
    with torch.no_grad():
        for d, sfx in enumerate(("", "_reverse")):
            wih = np.zeros((4 * H, 8 * H))
            wih[:, d * 4 * H:(d + 1) * 4 * H] = eye
            getattr(lstm, "weight_ih_l0" + sfx).copy_(torch.from_numpy(wih))
            getattr(lstm, "weight_hh_l0" + sfx).copy_(torch.from_numpy(W[d]))
            getattr(lstm, "bias_ih_l0" + sfx).zero_()
            getattr(lstm, "bias_hh_l0" + sfx).zero_()
    xin = torch.from_numpy(np.concatenate(x, 2)).requires_grad_(True)
    out, _ = lstm(xin)
    loss = sum((out[:, :, d * H:(d + 1) * H] * torch.from_numpy(dh[d])).sum() for d in use)
    loss.backward()
    for d in use:
        gates, c, h = R.run_fwd(x[d], W[d], reverse=d)
        _relclose(h, out[:, :, d * H:(d + 1) * H].detach().numpy(), f"h dir {d}")
        # c per frame: the final cell state of the sequence cut at that frame
        for t in range(T):
            with torch.no_grad():
                _, (_, cn) = lstm(xin[:t + 1] if d == 0 else xin[t:])
            _relclose(c[t], cn[d].numpy(), f"c[{t}] dir {d}")
        dG, _ = R.run_bwd(dh[d], W[d], gates, c, reverse=d)
        _relclose(dG, xin.grad[:, :, d * 4 * H:(d + 1) * 4 * H].numpy(), f"dgates dir {d}")
        sfx = "_reverse" if d else ""
        for name in ("bias_ih_l0", "bias_hh_l0"):
            _relclose(dG.sum((0, 1)), getattr(lstm, name + sfx).grad.numpy(), f"{name}{sfx}")


# ------------------------------------------------------------------ 2. the bounds on an fp32 restatement
@pytest.mark.parametrize("fma", [False, True], ids=["mul-add", "fma"])
@pytest.mark.parametrize("mode", [R.MODE_F32, R.MODE_BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H", [64, 128, 512])
def test_fp32_restatement_stays_inside_the_bounds(H, mode, fma):
    N, T = 5, 4
    for reverse in (0, 1):
        e = R.make_entry(H, N, T, seed=H + reverse)
        s16 = mode == R.MODE_BF16 and reverse == 1                   # bf16 storage of h / dG on one of the two runs
        dev, steps = R.run_f32(e, reverse, mode, fma, h_bf16=s16, g_bf16=s16)
        for dc_steps in (steps, None):
            res = R.check_dir(e["x"], e["W"], e["dh"], reverse, mode, dev, h_bf16=s16, g_bf16=s16, dc_steps=dc_steps)
            assert set(res) == {"gates", "a_rms", "exact", "c", "h", "dgates", "dh_rms", "dc"}
            print(f"H={H} mode={mode} fma={fma} reverse={reverse} stepped={dc_steps is not None}: " +
                  ", ".join(f"{k} {r:.3f}" for k, (r, _) in res.items()))
            for k, (r, where) in res.items():
                assert r <= 1.0, (k, r, where)
        db = (e["db0"][0].astype(F64) + dev["dG"].astype(F64).sum((0, 1))).astype(F)
        assert _worst(R.bias_check(dev["dG"], e["db0"][0], db)) <= 1.0
        slabs = np.zeros((16, 4 * H), F)
        slabs[0] = dev["dG"].astype(F64).sum((0, 1)).astype(F)
        assert _worst(R.bias_check(dev["dG"], None, None, slabs=slabs)) <= 1.0


def test_every_unit_class_is_in_every_tile_and_does_what_it_is_for():
    H, N, T = 64, 5, 4
    e = R.make_entry(H, N, T, seed=1)
    gates, c, h = R.run_fwd(e["x"], e["W"], 0)
    j = np.arange(H)
    for b in range(H // 16):
        assert {3, 7, 11} <= set(j[16 * b:16 * b + 16] % 16)
    assert (np.abs(c[-1][1:, j % 16 == 3]) > T - 0.1).all()                      # the cell integrates: tanh(c) saturates
    g7 = gates[:, 1:, np.concatenate([q * H + j[j % 16 == 7] for q in range(4)])]
    assert (np.abs(g7 - np.round(g7)) < 1e-35).all()                             # 0, 1 or +-1 to 1e-35: exactly so in fp32
    assert (np.abs(gates[0][:, 2 * H + j[j % 16 == 11]]) < 2.1e-4).all()         # tanh near 0 (the first frame: no recurrent term)
    assert (e["x"][0, 0] == 0).all() and (e["x"][-1, 0] == 0).all() and (e["dh"][:, 2] == 0).all()
    assert np.abs(e["W"][2 * H + 16:2 * H + 32]).max() > 4 / np.sqrt(H)


# ------------------------------------------------------------------ 3. mutations
H_M, N_M, T_M = 64, 5, 4


def _clean(reverse=0, mode=R.MODE_F32, seed=3):
    e = R.make_entry(H_M, N_M, T_M, seed)
    dev, steps = R.run_f32(e, reverse, mode, fma=False)
    return e, dev, steps


def _check(e, dev, reverse=0, mode=R.MODE_F32, dc_steps=None, **kw):
    return R.check_dir(e["x"], e["W"], e["dh"], reverse, mode, dev, dc_steps=dc_steps, **kw)


def test_mutation_one_element_of_h_moved_by_three_bounds():
    e, dev, steps = _clean()
    assert _worst(_check(e, dev, dc_steps=steps)) <= 1.0
    t, n, j = 2, 3, 20
    o = float(dev["gates"][t, n, 3 * H_M + j])
    tol = abs(o) * R.GATE_TANH_ABS * R.EPS32 + R.EPS32 * abs(float(dev["h"][t, n, j]))
    dev["h"][t, n, j] += F(3 * tol)
    assert float(dev["h"][t, n, j]) != o * np.tanh(float(dev["c"][t, n, j]))
    res = _check(e, dev, passes="f")
    assert res["h"][0] > 1.0 and "frame 2" in res["h"][1]


def test_mutation_f_and_g_gates_swapped():
    e, _, _ = _clean()
    sw = dict(e)
    H = H_M
    sw["x"] = np.concatenate([e["x"][..., :H], e["x"][..., 2 * H:3 * H], e["x"][..., H:2 * H], e["x"][..., 3 * H:]], -1)
    sw["W"] = np.concatenate([e["W"][:H], e["W"][2 * H:3 * H], e["W"][H:2 * H], e["W"][3 * H:]], 0)
    dev, _ = R.run_f32(sw, 0, R.MODE_F32, fma=False)             # a device that takes the order i, g, f, o
    res = _check(e, dev)
    assert res["gates"][0] > 1.0


def test_mutation_a_frame_computed_from_h_two_frames_back():
    e, dev, _ = _clean()
    t = 3
    gt, c, h = R.fwd_f32(e["x"][t], e["W"], dev["h"][t - 2], dev["c"][t - 1], R.MODE_F32, False)
    dev["gates"][t], dev["c"][t], dev["h"][t] = gt, c, h
    res = _check(e, dev, passes="f")
    assert res["gates"][0] > 1.0 and "frame 3" in res["gates"][1]


def test_mutation_reverse_ignored():
    e, dev, steps = _clean(reverse=0)
    res = _check(e, dev, reverse=1, dc_steps=steps)
    assert res["gates"][0] > 1.0 and res["dgates"][0] > 1.0


def test_mutation_dc_carry_dropped():
    e, dev, _ = _clean()
    o, dG = R.order(T_M, 0), dev["dG"].copy()
    zero = np.zeros((N_M, H_M), F)
    steps = []
    for s in range(T_M - 1, -1, -1):
        t, tp, tn = o[s], (o[s - 1] if s else None), (o[s + 1] if s + 1 < T_M else None)
        dG[t], dcar = R.bwd_f32(e["dh"][t], e["W"], None if tn is None else dG[tn], dev["gates"][t], dev["c"][t],
                                None if tp is None else dev["c"][tp], zero, R.MODE_F32, False)
        steps.append(dcar)
    dev["dG"] = dG
    assert _check(e, dev, passes="b")["dgates"][0] > 1.0                       # whole-sequence form: the reference's own carry
    # stepped form: dc_ws itself is right after every step, the frames did not take it
    assert _check(e, dev, passes="b", dc_steps=steps)["dgates"][0] > 1.0


def test_mutation_one_row_missing_from_a_bias_column_sum():
    e, dev, _ = _clean()
    dG = dev["dG"].astype(F64)
    full = e["db0"][0].astype(F64) + dG.sum((0, 1))
    assert _worst(R.bias_check(dev["dG"], e["db0"][0], full.astype(F))) <= 1.0
    short = (full - dG[1, N_M - 1]).astype(F)
    assert _worst(R.bias_check(dev["dG"], e["db0"][0], short)) > 1.0
    slabs = np.zeros((16, 4 * H_M), F)
    slabs[0] = (dG.sum((0, 1)) - dG[1, N_M - 1]).astype(F)
    assert R.bias_check(dev["dG"], None, None, slabs=slabs)["dbias_part"][0] > 1.0
    slabs[0] = dG.sum((0, 1)).astype(F)
    slabs[5, 7] = 1e-30                                                        # a row group the launch cannot have
    assert R.bias_check(dev["dG"], None, None, slabs=slabs)["dbias_part_zero_rows"][0] > 1.0


def _exact_product(a, b, add):
    return (np.asarray(a, F64) @ np.asarray(b, F64) + np.asarray(add, F64)).astype(F)


def _two_plane_product(a, b, add):
    """fp32x3 with the third split term of either operand lost."""
    a1, a2, _ = R.split3(a)
    b1, b2, _ = R.split3(b)
    return ((a1.astype(F64) + a2) @ (b1.astype(F64) + b2) + np.asarray(add, F64)).astype(F)


@pytest.mark.parametrize("H", [64, 1024])
def test_mutation_third_bf16_split_term_dropped_fails_the_rms_condition(H):
    N, T = 5, 2
    e = R.make_entry(H, N, T, seed=H)
    o = R.order(T, 0)
    for product, flagged in ((_exact_product, False), (_two_plane_product, True)):
        dev = {k: np.zeros((T, N, w), F) for k, w in (("gates", 4 * H), ("c", H), ("h", H))}
        for s, t in enumerate(o):
            tp = o[s - 1] if s else None
            dev["gates"][t], dev["c"][t], dev["h"][t] = R.fwd_f32(
                e["x"][t], e["W"], None if tp is None else dev["h"][tp], None if tp is None else dev["c"][tp],
                R.MODE_F32X3, False, product)
        res = R.check_dir(e["x"], e["W"], e["dh"], 0, R.MODE_F32X3, dev, passes="f")
        print(f"H={H} {product.__name__}: " + ", ".join(f"{k} {r:.3f}" for k, (r, _) in res.items()))
        assert (res["a_rms"][0] > 1.0) == flagged, res


def test_mutation_bf16_mode_product_with_an_unrounded_operand():
    e, dev, steps = _clean(mode=R.MODE_F32)                       # h[tp] and dG[tn] went in unrounded
    res = _check(e, dev, mode=R.MODE_BF16, dc_steps=steps)
    assert res["gates"][0] > 1.0 and res["dgates"][0] > 1.0
    e, dev, steps = _clean(mode=R.MODE_BF16)
    assert _worst(_check(e, dev, mode=R.MODE_BF16, dc_steps=steps)) <= 1.0


# ------------------------------------------------------------------ 4. which kernel a case reaches
CUS = 256                                             # compute units of the MI355X (pers_cu_count)


def dispatch(c):
    """The kernels csrc/lstm.hip / csrc/lstm_pers.hip launch for a case: the dispatch arithmetic restated."""
    ndir, H, N = len(c.rev), c.H, c.N
    if c.fam == "pers":
        assert ndir == 1 and H in (512, 1024)
        x3_ok = -(-N // 32) <= 4 and (H // 16) * -(-N // 32) <= CUS           # pers_x3_ok
        mt = next((m for m in (1, 2) if -(-N // (16 * m)) <= 16 and (H // 32) * -(-N // (16 * m)) <= CUS), 0)   # pers_mt
        out = []
        if c.mode == R.MODE_BF16:
            assert mt
            out.append(f"pers_fwd_bf16<{H},{mt}>")
        else:
            assert c.mode == R.MODE_F32X3 and x3_ok and not c.st16
            units = 8 if H == 512 and (H // 8) * -(-N // 32) <= CUS else 16    # dvae_pers_fwd_units
            out.append(f"pers_fwd_x3{'h' if units == 8 else ''}<{H}>")
        for b in c.bwd:
            if b == R.MODE_BF16:
                out.append(f"pers_bwd_bf16<{H},{mt}>")
            elif b == R.MODE_F32:
                assert x3_ok
                out.append(f"pers_bwd_f32<{H}>")
            else:
                assert x3_ok
                rows16 = H == 512 and (H // 16) * -(-N // 32) * 2 <= CUS and -(-N // 16) <= 8 and (H // 16) * -(-N // 16) <= CUS
                out.append(f"pers_bwd_x3k<{H}>" if H == 1024 else f"pers_bwd_x3<{H},{'16' if rows16 else '32'} rows>")
        return out
    if H == 64:
        rows = 16
        if c.mode:
            if -(-N // 8) * ndir <= 64:
                rows = 8
            if -(-N // 4) * ndir <= 64:
                rows = 4
        assert not any(c.shifts) and not c.st16
        return [f"h64<{c.mode},{rows}>"]
    assert not c.gld2
    if H % 512 == 0:
        n_j = H // 16
        mt5 = 2 if n_j * -(-N // 32) * ndir >= 256 else 1                      # plan_seq
        shifted = any(c.shifts)
        if c.mode == R.MODE_BF16:
            f, b = f"fwd_v5<{mt5},128,1,s16={c.st16}>", f"bwd_v5<{mt5},64,1,s16={c.st16}>"
        elif c.mode == R.MODE_F32X3:
            f, b = f"fwd_v5<{mt5},64,2>", f"bwd_v5<{mt5},{32 if mt5 == 2 else 64},2>"
        else:
            f = f"fwd_v5<2,{64 if shifted else 128},0>" if mt5 == 2 else "fwd_v5<1,64,0>"
            b = f"bwd_v5<{mt5},64,0>"
        return [f, b, f"n_m5={-(-N // (16 * mt5))}"]
    assert H % 64 == 0 and c.mode == R.MODE_F32 and not any(c.shifts)
    return [f"gen<k-chunks={H // 64},{'xcd' if (H // 16) % 8 == 0 else 'plain'} decode,n_m={-(-N // 16)}>"]


def test_every_case_reaches_the_kernel_its_note_names():
    got = {R.case_id(c): dispatch(c) for c in R.CASES}
    assert len(got) == len(R.CASES), "case ids are not unique"
    want = {
        "gen-fp32-H128-N17-T3-f": ["gen<k-chunks=2,xcd decode,n_m=2>"],
        "gen-fp32-H192-N33-T4-fxr": ["gen<k-chunks=3,plain decode,n_m=3>"],
        "gen-fp32-H128-N1-T1-f": ["gen<k-chunks=2,xcd decode,n_m=1>"],
        "h64-fp32-H64-N20-T5-fxr": ["h64<0,16>"],
        "h64-fp32-H64-N1-T1-f": ["h64<0,16>"],
        "pers-bf16-s16-H512-N40-T6-f": ["pers_fwd_bf16<512,1>", "pers_bwd_bf16<512,1>"],
        "pers-bf16-H1024-N129-T5-f": ["pers_fwd_bf16<1024,2>", "pers_bwd_bf16<1024,2>"],
        "pers-fp32x3-H1024-N17-T6-f": ["pers_fwd_x3<1024>", "pers_bwd_x3k<1024>", "pers_bwd_f32<1024>"],
        "pers-fp32x3-H512-N97-T7-r": ["pers_fwd_x3h<512>", "pers_bwd_x3<512,16 rows>", "pers_bwd_f32<512>"],
    }
    for m, name in ((R.MODE_F32X3, "fp32x3"), (R.MODE_BF16, "bf16")):
        for N, rows in ((5, 4), (130, 8), (258, 16)):
            want[f"h64-{name}-H64-N{N}-T3-fxr"] = [f"h64<{m},{rows}>"]
    for name, fk, bk in (("fp32", "{mt},{kr},0", "{mt},64,0"), ("fp32x3", "{mt},64,2", "{mt},{bkr},2"),
                         ("bf16", "{mt},128,1,s16=0", "{mt},64,1,s16=0"), ("bf16-s16", "{mt},128,1,s16=1", "{mt},64,1,s16=1")):
        for shape, mt, n_m, shifted in (("H512-N17-T4-r", 1, 2, 0), ("H1024-N97-T3-f", 2, 4, 0), ("H512-N97-T3-fxr", 2, 4, 0),
                                        ("H1024-N97-T4-fxf-shift", 2, 4, 1)):
            kr = 64 if (mt == 1 or shifted) else 128
            want[f"v5-{name}-{shape}"] = [f"fwd_v5<{fk.format(mt=mt, kr=kr)}>", f"bwd_v5<{bk.format(mt=mt, bkr=32 if mt == 2 else 64)}>",
                                          f"n_m5={n_m}"]
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    # the ragged tails the notes speak of
    assert 97 % 32 == 1 and 130 % 8 == 2 and 17 % 16 == 1 and 129 % 32 == 1
    for c in R.CASES:
        if c.fam == "pers":
            assert c.T >= 5, "the two-slot exchange ring wraps twice from T = 5"
