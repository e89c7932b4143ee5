"""The float64 reference of the batch-norm kernels (tests/bn_ref.py), proved without a GPU.

1. `bn_ref` against torch.nn.BatchNorm1d in float64, one module call per group in group order (what the reference model
   does with the two utterances of a pair): forward, running_mean, running_var, num_batches_tracked and autograd's dx,
   dweight, dbias to 1e-12 relative, for act none / ReLU / tanh, G = 1 and 2, and the residual form x + bn(x).
2. The kernel's rule at one value per channel and group (torch refuses that input).
3. The rounding bounds of tests/bn_ref.py on a numpy float32 restatement of the kernels' statements (mean and rstd
   already rounded to fp32; with and without fused multiply-adds) on the very inputs tests/test_hip_bn.py uploads: the
   worst error / bound per quantity is printed and must stay below 1 — the derivation is checked before a GPU is asked.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_ref as B  # noqa: E402

ACTS = {"none": B.ACT_NONE, "relu": B.ACT_RELU, "tanh": B.ACT_TANH}
TORCH_ACT = {B.ACT_NONE: lambda t: t, B.ACT_RELU: torch.relu, B.ACT_TANH: torch.tanh}


def _relclose(a, b, what, rel=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    bad = np.abs(a - b) > rel * np.abs(b) + 1e-300
    assert a.shape == b.shape and not bad.any(), (what, int(bad.sum()), a[bad][:3], b[bad][:3])


def _torch_run(d, N, G, act, eps, momentum, residual):
    """One BatchNorm1d module in float64, called once per group in group order.  Returns z, running statistics, the call
    count and autograd's gradients, rows put back where the frame-major layout has them."""
    y = d["y"].astype(np.float64)
    R, C = y.shape
    gi = B.groups(R, N, G)
    bn = torch.nn.BatchNorm1d(C, eps=eps, momentum=momentum).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(d["gamma"].astype(np.float64)))
        bn.bias.copy_(torch.from_numpy(d["beta"].astype(np.float64)))
        bn.running_mean.copy_(torch.from_numpy(d["rm0"].astype(np.float64)))
        bn.running_var.copy_(torch.from_numpy(d["rv0"].astype(np.float64)))
    x = torch.from_numpy(y.copy()).requires_grad_()
    z = torch.zeros(R, C, dtype=torch.float64)
    for k in range(G):
        rows = torch.from_numpy(np.nonzero(gi == k)[0])
        zk = TORCH_ACT[act](bn(x[rows]))
        if residual:
            zk = x[rows] + zk
        z = z.index_copy(0, rows, zk)
    (z * torch.from_numpy(d["dz"].astype(np.float64))).sum().backward()
    return (z.detach().numpy(), bn.running_mean.numpy(), bn.running_var.numpy(), int(bn.num_batches_tracked),
            x.grad.numpy(), bn.weight.grad.numpy(), bn.bias.grad.numpy())


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("eps,momentum", [(1e-5, 0.1), (1e-3, 0.5)])
def test_reference_is_torch_batchnorm_in_float64(act, G, eps, momentum):
    R, N, C = 126, 6, 20
    d = B.make_inputs(R, N, G, C, seed=3)
    a = ACTS[act]
    z_t, rm_t, rv_t, nbt, dx_t, dw_t, db_t = _torch_run(d, N, G, a, eps, momentum, residual=False)
    mean, var, rstd = B.stats(d["y"], N, G, eps)
    rm, rv = B.running(d["rm0"], d["rv0"], mean, var, B.count(R, N, G), momentum)
    u, z = B.apply(d["y"], mean, rstd, d["gamma"], d["beta"], None, N, G, a)
    _relclose(z, z_t, "z")
    _relclose(rm, rm_t, "running_mean")
    _relclose(rv, rv_t, "running_var")
    assert nbt == G
    for from_z in (True, False):
        if not from_z and a == B.ACT_TANH:
            continue
        _, s1, s2, dgamma, dbeta, dy = B.bwd(d["dz"], d["y"], z if from_z else None, mean, rstd, d["gamma"], d["beta"], N, G, a)
        _relclose(dy, dx_t, f"dx (from_z={from_z})")
        _relclose(dgamma, dw_t, "dweight")
        _relclose(dbeta, db_t, "dbias")


@pytest.mark.parametrize("G", [1, 2])
def test_reference_residual_form_is_x_plus_bn_x(G):
    R, N, C = 126, 6, 20
    d = B.make_inputs(R, N, G, C, seed=4)
    z_t, *_ = _torch_run(d, N, G, B.ACT_NONE, 1e-5, 0.1, residual=True)
    mean, var, rstd = B.stats(d["y"], N, G, 1e-5)
    _, z = B.apply(d["y"], mean, rstd, d["gamma"], d["beta"], d["y"], N, G, B.ACT_NONE)
    _relclose(z, z_t, "x + bn(x)")
    for name, a in ACTS.items():                               # the ABI's act(u) + residual
        u, z = B.apply(d["y"], mean, rstd, d["gamma"], d["beta"], d["res"], N, G, a)
        assert np.array_equal(z, B.act_apply(u, a) + d["res"].astype(np.float64)), name


def test_one_value_per_channel_and_group_uses_the_biased_variance():
    """cnt == 1: mean = y, var = 0, rstd = eps^-1/2, and the running variance moves towards 0 (the biased variance; the
    unbiased one would divide by zero).  torch raises for this input, so the kernel's rule is what is pinned."""
    d = B.make_inputs(2, 2, 2, 4, seed=5)
    mean, var, rstd = B.stats(d["y"], 2, 2, 1e-5)
    assert np.array_equal(mean, d["y"].astype(np.float64)) and not var.any()
    _relclose(rstd, np.full((2, 4), 1e-5 ** -0.5), "rstd")
    rm, rv = B.running(d["rm0"], d["rv0"], mean, var, 1, 0.1)
    _relclose(rv, 0.81 * d["rv0"].astype(np.float64), "running_var")
    _relclose(rm, 0.9 * (0.9 * d["rm0"].astype(np.float64) + 0.1 * mean[0]) + 0.1 * mean[1], "running_mean")
    with pytest.raises(ValueError):
        torch.nn.BatchNorm1d(4).double()(torch.from_numpy(d["y"][:1].astype(np.float64)))


def test_group_rule_and_tree_counts():
    assert B.groups(8, 4, 2).tolist() == [0, 0, 1, 1, 0, 0, 1, 1] and B.count(8, 4, 2) == 4
    assert B.tree_adds(64) == 27 and B.var_roundings(64) == 86 and B.tree_adds(16400) == 31
    assert B.tree_adds(64 * 1025, from_partials=True) == 64 + 7 + 17
    # the kappa up to which the cancellation term of rstd stays below one fp32 rounding (module docstring of bn_ref)
    assert 1.2e7 < 2.0 ** 30 / B.var_roundings(64) < 1.3e7


# ------------------------------------------------------------------ the bounds, on an fp32 restatement
def _note(worst, key, got, ref, tol, skip=None):
    if skip is not None:
        keep = ~np.broadcast_to(skip, np.shape(ref))
        got, ref, tol = np.asarray(got)[keep], np.asarray(ref)[keep], np.broadcast_to(tol, np.shape(ref))[keep]
    worst[key] = max(worst.get(key, 0.0), B.worst_ratio(got, ref, tol)[0])


@pytest.mark.parametrize("case", B.CASES, ids=lambda c: "x".join(map(str, c)))
def test_fp32_restatement_meets_the_bounds_on_the_gpu_tests_inputs(case):
    R, N, G, C = case
    d = B.make_inputs(R, N, G, C, B.SEEDS[case])
    eps, mom = np.float32(1e-5), np.float32(0.1)
    sb = B.stats_bounds(d["y"], N, G, eps, d["rm0"], d["rv0"], mom)
    mean32, rstd32 = sb["mean"].astype(np.float32), sb["rstd"].astype(np.float32)
    cnt = B.count(R, N, G)
    unb = sb["var"] * cnt / (cnt - 1.0) if cnt > 1 else sb["var"]
    worst = {}
    _note(worst, "mean", mean32, sb["mean"], sb["tol_mean"])
    _note(worst, "rstd", rstd32, sb["rstd"], sb["tol_rstd"])
    amb = B.ambiguous_pairs(d["y"], mean32, rstd32, d["gamma"], d["beta"], N, G)
    assert not amb.any(), f"seed {B.SEEDS[case]} leaves {int(amb.sum())} ambiguous (group, channel) pairs: choose another"
    for fma in (False, True):
        _note(worst, "running_mean", B.running_f32(d["rm0"], sb["mean"], mom, fma), sb["rm"], sb["tol_rm"])
        _note(worst, "running_var", B.running_f32(d["rv0"], unb, mom, fma), sb["rv"], sb["tol_rv"])
        for name, a in ACTS.items():
            for res in (None, d["res"]):
                ab = B.apply_bounds(d["y"], mean32, rstd32, d["gamma"], d["beta"], res, N, G, a)
                z = B.apply_f32(d["y"], mean32, rstd32, d["gamma"], d["beta"], res, N, G, a, fma)
                _note(worst, "z_" + name, z, ab["z"], ab["tol_z"])
                if res is not None:
                    continue
                for from_y in (False, True):
                    if from_y and a == B.ACT_TANH:
                        continue
                    zin = None if from_y else z
                    s12, dg, db, dy = B.bwd_f32(d["dz"], d["y"], zin, mean32, rstd32, d["gamma"], d["beta"], N, G, a,
                                                d["dgamma0"], d["dbeta0"], fma)
                    bb = B.bwd_bounds(d["dz"], d["y"], zin, mean32, rstd32, d["gamma"], d["beta"], N, G, a,
                                      d["dgamma0"], d["dbeta0"], s12=s12)
                    _note(worst, "s1", s12[..., 0], bb["s1"], bb["tol_s1"])
                    _note(worst, "s2", s12[..., 1], bb["s2"], bb["tol_s2"])
                    _note(worst, "dgamma", dg, bb["dgamma"], bb["tol_dgamma"])
                    _note(worst, "dbeta", db, bb["dbeta"], bb["tol_dbeta"])
                    _note(worst, "dy", dy, bb["dy"], bb["tol_dy"])
    print(f"fp32 restatement {R}x{C} N={N} G={G}, worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) < 1.0, worst


def _tree_sum(x):
    """The float64 sum over the rows of x [R, C] in the order of bn_partial_kernel + sum_partials: per 64-row chunk four row
    lanes of 16 rows each, added in turn, then the lanes; thread kl adds the chunks kl, kl + 64, ... in turn; four shuffle
    levels over 16 threads, then four waves.  (numpy's own axis-0 sum adds the rows in turn: R additions per term.)"""
    R, C = x.shape
    ch = B.n_chunks(R)
    p = np.zeros((-(-ch // 64) * 64 * 64, C))
    p[:R] = x
    p = p.reshape(-1, 16, 4, C)                       # chunk, trip, row lane
    lane = np.zeros((p.shape[0], 4, C))
    for t in range(16):
        lane = lane + p[:, t]
    part = ((lane[:, 0] + lane[:, 1]) + lane[:, 2]) + lane[:, 3]
    part = part.reshape(-1, 64, C)                    # trip over chunks, kl
    s = np.zeros((64, C))
    for t in range(part.shape[0]):
        s = s + part[t]
    s = s.reshape(4, 16, C)                           # wave, kl & 15
    for off in (1, 2, 4, 8):
        s = s + s[:, np.arange(16) ^ off]
    return ((s[0, 0] + s[1, 0]) + s[2, 0]) + s[3, 0]


def test_cancellation_bound_on_the_restated_one_pass_variance():
    """E[y^2] - E[y]^2 in float64, summed in the kernel's order, on the cancellation inputs: mean and rstd, rounded to fp32,
    inside tol_mean / tol_rstd at every kappa, the constant channel included."""
    y = B.cancellation_inputs().astype(np.float64)
    sb = B.stats_bounds(y, 1, 1, np.float32(1e-5))
    m = _tree_sum(y) / len(y)
    var = np.maximum(_tree_sum(y * y) / len(y) - m * m, 0.0)
    rstd = (1.0 / np.sqrt(var + float(np.float32(1e-5)))).astype(np.float32)
    rm, _ = B.worst_ratio(m.astype(np.float32), sb["mean"][0], sb["tol_mean"][0])
    rr, _ = B.worst_ratio(rstd, sb["rstd"][0], sb["tol_rstd"][0])
    print("kappa " + " ".join(f"{k:.2g}" for k in sb["kappa"][0]) + " | cancellation term / eps32 "
          + " ".join(f"{k:.2g}" for k in sb["rstd_cancel_over_eps32"][0]) + f" | worst error / bound: mean {rm:.3f} rstd {rr:.3f}")
    assert rm < 1.0 and rr < 1.0
    # worst case below one fp32 rounding up to |mean|/std = 1e3 (offset 10), what the model reaches; above it no longer
    assert (sb["rstd_cancel_over_eps32"][0][:3] < 1.0).all() and (sb["rstd_cancel_over_eps32"][0][3:] > 1.0).all()


def test_exact_zero_case_is_exact_in_the_fp32_restatement():
    """The exact-zero case of tests/test_hip_bn.py is compared bit for bit on the device: every statement is exact on that
    data, so the fp32 restatement, with and without fused multiply-adds, must equal the rounded float64 reference."""
    R, C, y, gamma, beta, dz = B.exact_zero_case()
    mean, rstd, zero = np.full((1, C), 0.5, np.float32), np.full((1, C), 2.0, np.float32), np.zeros(C, np.float32)
    u, _ = B.apply(y, mean, rstd, gamma, beta, None, 1, 1, B.ACT_NONE)
    assert set(np.unique(u)) == {-2.0 ** -23, -2.0 ** -24, 0.0, 2.0 ** -24, 2.0 ** -23}
    for a in (B.ACT_NONE, B.ACT_RELU):
        for fma in (False, True):
            z = B.apply_f32(y, mean, rstd, gamma, beta, None, 1, 1, a, fma)
            assert np.array_equal(z.astype(np.float64), B.act_apply(u, a))
            for zin in (z, None):
                s12, dg, db, dy = B.bwd_f32(dz, y, zin, mean, rstd, gamma, beta, 1, 1, a, zero, zero, fma)
                _, s1, s2, dgam, dbet, dyr = B.bwd(dz, y, zin, mean, rstd, gamma, beta, 1, 1, a)
                assert np.array_equal(s12[0, :, 0], s1[0].astype(np.float32)) and np.array_equal(s12[0, :, 1], s2[0].astype(np.float32))
                assert np.array_equal(dg, dgam.astype(np.float32)) and np.array_equal(db, dbet.astype(np.float32))
                assert np.array_equal(dy, dyr.astype(np.float32)) and dy.any()
