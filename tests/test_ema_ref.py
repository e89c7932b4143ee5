"""The float64 reference of the weight average (tests/ema_ref.py), proved without a GPU: it is the closed form of an
exponential moving average with and without warm-up, it is torch.optim.swa_utils' EMA in float64 where the installed torch
has one, and the bound the sweep is held to (tests/test_hip_ema.py) holds for an fp32 restatement of the kernel in numpy and
tells an fma from a product rounded on its own.  Also the host side of the feature: the command-line flags, the file-name
rule that keeps `<epoch>.ema.pth` from being taken for a checkpoint, and what FlatAdam.set_ema refuses."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dvae_amd  # noqa: E402,F401
from adam_ref import grad_mixture, params  # noqa: E402
from ema_ref import (EPS32, TICK_REL, closed_form, decay_at, ema_update_f32, ema_update_ref, tick_ref, update_bounds,  # noqa: E402
                     weight_at, worst_ratio)


def _iterates(n, steps, seed=0):
    """p_0 .. p_steps: weights that move like an optimiser's (a drift of 1e-3 per step on values in [-1, 1])"""
    p = params(seed, n).astype(np.float64)
    out = [p]
    for j in range(steps):
        out.append(out[-1] - 1e-3 * np.sign(grad_mixture(seed + 1 + j, n).astype(np.float64)))
    return out


@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warm-up"])
@pytest.mark.parametrize("decay", [0.0, 0.5, 0.9, 0.999])
def test_reference_is_the_closed_form(decay, warmup):
    n, steps = 512, 25
    ps = _iterates(n, steps)
    e, k, ds = ps[0].copy(), 0, []
    for j in range(1, steps + 1):
        k, w, applied = tick_ref(k, decay, warmup)
        assert k == j and applied == 1 and w == 1.0 - decay_at(decay, j, warmup)
        ds.append(decay_at(decay, j, warmup))
        e = ema_update_ref(e, ps[j], w)
    want = closed_form(ps[0], ps[1:], ds)
    assert np.abs(e - want).max() <= 64 * 2.0 ** -53 * np.abs(want).max()
    d32 = float(np.float32(decay))
    if warmup:
        assert ds[0] == min(d32, 2.0 / 11.0) and all(d <= d32 for d in ds)
        late = [j for j in range(1, steps + 1) if (1.0 + j) / (10.0 + j) >= d32]
        assert all(ds[j - 1] == d32 for j in late)                      # the ramp hands over to the decay and stays there
    else:
        assert all(d == d32 for d in ds)
    if decay == 0.0:
        assert np.array_equal(e, ps[-1])                                # no memory: the average IS the last iterate


def test_skipped_tick_changes_nothing():
    assert tick_ref(7, 0.9, True, skipped=True) == (7, None, 0)
    assert tick_ref(7, 0.9, True) == (8, weight_at(0.9, 8, True), 1)


@pytest.mark.parametrize("decay", [0.5, 0.9, 0.999])
def test_reference_is_torch_swa_utils_ema_in_float64(decay):
    swa = torch.optim.swa_utils
    if not hasattr(swa, "get_ema_multi_avg_fn"):
        pytest.skip("this torch has no torch.optim.swa_utils.get_ema_multi_avg_fn")
    n, steps = 512, 12
    ps = _iterates(n, steps, seed=3)

    class One(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.from_numpy(ps[0].copy()))

    model = One()
    avg = swa.AveragedModel(model, multi_avg_fn=swa.get_ema_multi_avg_fn(float(np.float32(decay))))
    avg.update_parameters(model)                                        # the first call copies: e_0 = p_0
    e, k = ps[0].copy(), 0
    for j in range(1, steps + 1):
        with torch.no_grad():
            model.w.copy_(torch.from_numpy(ps[j]))
        avg.update_parameters(model)
        k, w, _ = tick_ref(k, decay, False)
        e = ema_update_ref(e, ps[j], w)
        got = avg.module.w.detach().numpy()
        assert np.abs(e - got).max() <= 1e-14 * np.abs(got).max(), j


@pytest.mark.parametrize("w", [1.0, 9.0 / 11.0, 0.1, 1e-3, 1e-4])
def test_fp32_restatement_meets_the_bound_and_the_bound_tells_an_fma(w):
    w = np.float32(w)
    worst, worst_unfused = 0.0, 0.0
    for seed, n in enumerate([4, 2044, 6208, 100003]):
        p = params(70 + seed, n)
        for spread in (1.0, 1e-3, 1e-6):              # the average far from, near, and within a few ulp of the weights
            e = (p.astype(np.float64) + spread * params(170 + seed, n)).astype(np.float32)
            e[::7] = p[::7]                            # and some elements equal bit for bit
            b = update_bounds(e, p, w)
            got = ema_update_f32(e, p, w)
            worst = max(worst, worst_ratio(got, b["ref"], b["tol"])[0])
            worst_unfused = max(worst_unfused, worst_ratio(ema_update_f32(e, p, w, fused=False), b["ref"], b["tol"])[0])
            assert np.array_equal(got[::7].view(np.uint32), e[::7].view(np.uint32))          # p == e keeps the bits
    print(f"fp32 restatement, w={float(w):.6g}: worst error / bound {worst:.3f} with an fma, {worst_unfused:.3f} without")
    assert 0.0 < worst <= 1.0
    assert worst_unfused <= 2.0                        # one more rounding of w s: at most eps32 w |p - e| on top


def test_bound_is_of_the_order_of_one_ulp_of_the_result():
    e, p = np.float32([0.5, -0.25, 1e-3]), np.float32([0.75, -0.26, 1e-3])
    b = update_bounds(e, p, np.float32(0.1))
    assert np.all(b["tol"] <= 2.2 * EPS32 * np.maximum(np.abs(b["ref"]), np.abs(e))) and np.all(b["tol"] > 0)
    assert TICK_REL == 2.0 ** -23


# ------------------------------------------------------------------ the host side of the feature
def test_train_cli_flags():
    from dvae_amd import train
    a = train.get_parse().parse_args([])
    assert a.ema_decay == 0.0 and a.use_ema is False                    # off unless asked for
    a = train.get_parse().parse_args(["--ema-decay", "0.999", "--use-ema"])
    assert a.ema_decay == 0.999 and a.use_ema is True
    for bad in ("1", "1.5", "-0.1", "nan"):
        with pytest.raises(SystemExit, match="--ema-decay"):            # refused before anything touches a device
            train.main(["--ema-decay", bad])


def test_probe_cli_flag():
    from dvae_amd import probe
    assert probe._parse(["corpus", "--log_dir", "run"]).use_ema is False
    assert probe._parse(["corpus", "--log_dir", "run", "--use-ema"]).use_ema is True


def test_ema_file_is_not_a_checkpoint_candidate(tmp_path):
    from dvae_amd import probe
    from dvae_amd.model.variational_base_vae import VariationalBaseModelVAE
    w = VariationalBaseModelVAE(None, 64, 80, 1, 32, 1e-3, "cpu", 500, 4)
    said = []
    (tmp_path / "X_Y_5.ema.pth").write_bytes(b"")
    assert probe.checkpoint_files(tmp_path) == []
    assert w.load_last_model(str(tmp_path), logging_func=said.append) == 1 and "from scratch" in said[0]
    assert w.load_last_model(str(tmp_path), logging_func=said.append, use_ema=True) == 1       # nothing to resume from either
    (tmp_path / "X_Y_5.pth").write_bytes(b"")
    (tmp_path / "X_Y_4.pth").write_bytes(b"")
    assert [os.path.basename(f) for f in probe.checkpoint_files(tmp_path)] == ["X_Y_4.pth", "X_Y_5.pth"]
    os.remove(tmp_path / "X_Y_5.ema.pth")
    (tmp_path / "X_Y_4.ema.pth").write_bytes(b"")                      # an older epoch's average does not stand in
    with pytest.raises(FileNotFoundError, match=r"X_Y_5\.ema\.pth"):
        w.load_last_model(str(tmp_path), logging_func=said.append, use_ema=True)


def test_set_ema_refuses_bad_decays_and_cpu_buffers():
    from dvae_amd.optim import FlatAdam
    opt = FlatAdam([("w", torch.nn.Parameter(torch.zeros(8)))])
    assert opt.ema is None and opt.ema_decay is None and opt.ema_swapped is False
    assert "ema" not in opt.state_dict()
    for bad in (1.0, 1.5, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="decay"):
            opt.set_ema(bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.set_ema(0.9)
    opt.set_ema(None)                                                   # off stays off
    for call in (opt.ema_stats, opt.swap_ema, opt.ema_weights):
        with pytest.raises(RuntimeError, match="never switched on"):
            with call():
                pass
    assert opt.ema is None and "ema" not in opt.state_dict()
