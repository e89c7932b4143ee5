"""The float64 reference of the latent, loss, reduction, activation and layout kernels (tests/elem_ref.py), proved without a GPU.

1. `elem_ref` against torch float64 autograd of the reference model's formulas (disentangled_vae.py:250-279, 310-327;
   variational_base_vae.py:281-301, 335-348): values and gradients, the detached x2 style head included, to float64 roundoff.
2. The rounding bounds of tests/elem_ref.py on a numpy float32 restatement of the kernels' operation order, on the very inputs
   tests/test_hip_elem.py uploads, with exp replaced by a float64 exp pushed to EXPF_ROUNDINGS roundings either way.
3. Seeded wrong restatements (a dropped term, a style gradient not halved, a skipped tail element, two swapped scales, a
   tie that gives -w, a lost row, a slab added twice) leave the bounds: they are not slack enough to hide these.
4. Every case of elem_ref.CASES reaches the path it is named for, by the launch arithmetic restated in elem_ref.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elem_ref as E  # noqa: E402

T64 = lambda a: torch.from_numpy(np.asarray(a, np.float64).copy())
PUSHES = (1.0, -1.0, 0.0)


def _relclose(a, b, what, rel=1e-12, atol=1e-300):
    """atol: float64 roundoff of a difference that cancels (1 - exp(lv) at |lv| ~ 2^-24 is exact to 2^-53 of 1, not of itself)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    bad = np.abs(a - b) > rel * np.abs(b) + atol
    assert a.shape == b.shape and not bad.any(), (what, int(bad.sum()), a[bad][:3], b[bad][:3])


def _inside(got, ref, tol, what):
    r, i = E.worst_ratio(got, ref, tol)
    assert r <= 1.0, f"{what}: error / bound = {r:.3f} at flat index {i}"
    return r


def _outside(got, ref, tol):
    return E.worst_ratio(got, ref, tol)[0] > 1.0


# ------------------------------------------------------------------ 1. the reference is the model's formulas
UPSTREAM = {"all": ("dz", "dq_mu", "dq_lv", "ds_mu", "ds_lv"), "dz_only": ("dz",), "no_dz": ("dq_mu", "dq_lv", "ds_mu", "ds_lv"),
            "no_ds": ("dz", "dq_mu", "dq_lv"), "none": ()}


def _narrow(d):
    """The same inputs with the log-variances folded into [-3, 3]: relative agreement to 1e-12 is asked of float64 there."""
    d = dict(d)
    for k, w in (("style", d["style"].shape[1] // 2), ("content", d["content"].shape[1] // 2)):
        d[k] = d[k].copy()
        d[k][:, w:] = np.clip(d[k][:, w:], -3, 3)
    return d


@pytest.mark.parametrize("with_eps_c", [True, False])
@pytest.mark.parametrize("up", list(UPSTREAM))
def test_latent_reference_is_the_models_forward_in_float64(up, with_eps_c):
    Bh, S, Cn = 5, E.MODEL_S, E.MODEL_CN
    d = _narrow(E.latent_inputs(Bh, S, Cn, 11))
    st, co = T64(d["style"]).requires_grad_(), T64(d["content"]).requires_grad_()
    smu1, slv1, smu2, slv2 = st[:Bh, :S], st[:Bh, S:], st[Bh:, :S].detach(), st[Bh:, S:].detach()
    smu, slv = (smu1 + smu2) / 2, (slv1 + slv2) / 2
    rep = lambda mu, lv, e: e * torch.exp(0.5 * lv) + mu
    zs = rep(smu, slv, T64(d["eps_s"]))
    cmu, clv = co[:, :Cn], co[:, Cn:]
    zc = rep(cmu, clv, T64(d["eps_c"])) if with_eps_c else cmu
    z = torch.cat((torch.cat((zs, zs), 0), zc), -1)
    q_mu = torch.cat((torch.cat((smu, smu), 0), cmu), -1)
    q_lv = torch.cat((torch.cat((slv, slv), 0), clv), -1)
    eps_c = d["eps_c"] if with_eps_c else None
    got = E.latent_fwd(d["style"], d["content"], eps_c, d["eps_s"], Bh, S, Cn)
    for a, b, nm in zip(got, (z, q_mu, q_lv, smu, slv), ("z", "q_mu", "q_lv", "s_mu", "s_lv")):
        _relclose(a, b.detach().numpy(), nm, atol=1e-14)           # z = eps exp(lv / 2) + mu may cancel
    ups = {k: (d[k] if k in UPSTREAM[up] else None) for k in UPSTREAM["all"]}
    tot = sum((t * T64(ups[k])).sum() for k, t in (("dz", z), ("dq_mu", q_mu), ("dq_lv", q_lv), ("ds_mu", smu), ("ds_lv", slv))
              if ups[k] is not None)
    if up != "none":
        tot.backward()
    zero = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
    ds, dc = E.latent_bwd(d["style"], d["content"], eps_c, d["eps_s"], ups["dz"], ups["dq_mu"], ups["dq_lv"], ups["ds_mu"], ups["ds_lv"], Bh, S, Cn)
    _relclose(ds, zero(st), "dstyle", 1e-11, 1e-15)
    _relclose(dc, zero(co), "dcontent", 1e-11, 1e-15)
    assert not ds[Bh:].any()                                                   # the detached head


def test_loss_reference_is_loss_functionGVAE2_in_float64():
    B_, n, nq, ns = 5, 1023, 255, 300
    d = E.loss_inputs(n, nq, ns, "R", 3, wide=False)
    bs = 1.0 / float(d["l1_scale"])
    x = [T64(d["x1"]), T64(d["x2"])]
    r = [T64(d[k]).requires_grad_() for k in E.LOSS_KEYS[2:6]]
    q = [T64(d[k]).reshape(B_, -1).requires_grad_() for k in E.LOSS_KEYS[6:10]]
    s = [T64(d[k]).requires_grad_() for k in E.LOSS_KEYS[10:]]
    l1 = [F.l1_loss(x[k & 1], r[k], reduction="sum").div(bs) for k in range(4)]
    kl = lambda mu, lv: (-0.5) * torch.sum(1 + lv - mu.pow(2) - lv.exp(), axis=-1).mean()
    k1, k2 = kl(q[0], q[1]), kl(q[2], q[3])
    ks = (-1) * torch.sum(1 + s[1] - s[0].pow(2) - s[1].exp()).div(bs)
    loss = float(d["mse_cof"]) * (l1[0] + l1[1] + l1[2] + l1[3]) + float(d["kl_cof"]) * (k1 + k2)
    ref = torch.stack([loss, *l1, k1, k2, ks])
    d64 = dict(d, l1_scale=1.0 / bs, kl_scale=-0.5 / B_, style_scale=-1.0 / bs)
    # (the scalars of the descriptor are fp32: the float64 formulas are evaluated at those very values)
    ref_np = ref.detach().numpy()
    out = E.loss_fwd(d)
    fix = np.array([1.0, *[float(d["l1_scale"]) * bs] * 4, *[float(d["kl_scale"]) / (-0.5 / B_)] * 2, float(d["style_scale"]) * (-bs)])
    _relclose(out[1:], ref_np[1:] * fix[1:], "out[1..7]", 1e-11, 1e-12)
    _relclose(out[0], E.out0(list(out[1:]), d), "out[0]")
    for name, g8 in E.G8.items():
        for t in r + q + s:
            t.grad = None
        # gradients of the formulas at the descriptor's fp32 scalars: out[k] = fix[k] * ref[k]
        (ref[1:] * T64(fix[1:]) * T64(g8[1:])).sum().backward(retain_graph=True)
        g0 = float(g8[0])
        o0 = float(d["mse_cof"]) * sum(ref[1 + k] * fix[1 + k] for k in range(4)) + float(d["kl_cof"]) * (ref[5] * fix[5] + ref[6] * fix[6])
        (g0 * o0).backward(retain_graph=True)
        got = E.loss_bwd(d, g8.astype(np.float64))
        for a, t, nm in zip(got, r + q + s, E.LOSS_KEYS[2:]):
            _relclose(a, t.grad.numpy().reshape(-1), f"d{nm} ({name})", 1e-10, 1e-14)
    assert d64["n"] == n


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("scale", [-0.1, 0.25])
def test_kl_and_l1_references_against_autograd(n, scale):
    rs = np.random.RandomState(n)
    mu, lv = E.edge_mu(rs, n), E.edge_lv(rs, n, wide=False)
    m, l = T64(mu).requires_grad_(), T64(lv).requires_grad_()
    s32 = float(np.float32(scale))
    out = s32 * torch.sum(1 + l - m.pow(2) - l.exp())
    (out * 1.5).backward()
    _relclose(E.kl_fwd(mu, lv, scale), out.item(), "kl", 1e-11, 1e-12)
    dmu, dlv = E.kl_bwd(mu, lv, 1.5, s32)
    _relclose(dmu, m.grad.numpy(), "dmu")
    _relclose(dlv, l.grad.numpy(), "dlv", 1e-10, 1e-15)
    x, y = E.edge_pair(rs, n)
    yt = T64(y).requires_grad_()
    o = F.l1_loss(T64(x), yt, reduction="sum") * s32
    (o * 1.5).backward()
    _relclose(E.l1_fwd(x, y, scale), o.item(), "l1")
    assert np.array_equal(E.l1_bwd(x, y, 1.5, s32), yt.grad.numpy())            # torch's sign(0) = 0 at the ties


def test_activation_slab_colsum_conversion_references():
    rs = np.random.RandomState(5)
    for act, fn in ((E.ACT_NONE, lambda t: t), (E.ACT_RELU, torch.relu), (E.ACT_TANH, torch.tanh)):
        u = T64(rs.uniform(-2, 2, 300)).requires_grad_()
        dz = rs.uniform(-1, 1, 300)
        z = fn(u)
        z.backward(T64(dz))
        _relclose(E.act_bwd(dz, z.detach().numpy(), act), u.grad.numpy(), f"act_bwd {act}", 1e-10)
        c, _, slabs = E.slab_inputs(300, 5, 308, "R", 1)
        ref = fn(T64(c) + sum(T64(s_) for s_ in slabs)).numpy()
        got = E.slab_sum_f32(c, slabs, act, 1).astype(np.float64)
        assert np.abs(got - ref).max() < 1e-5
    Xm = rs.uniform(-1, 1, (37, 12))
    _relclose(E.colsum(Xm, 10, np.ones(10)), (T64(Xm)[:, :10].sum(0) + 1).numpy(), "colsum")
    n, m, S, Cn = 7, 3, 4, 28
    ss, sc, ts = rs.uniform(-1, 1, (n, 2 * S)), rs.uniform(-1, 1, (n, 2 * Cn)), rs.uniform(-1, 1, (m, 2 * S))
    src = torch.mean(T64(ss)[:, :S], axis=0, keepdim=True).repeat(n, 1)
    trg = torch.mean(T64(ts)[:, :S], axis=0, keepdim=True).repeat(n, 1)
    zs, zc = E.conversion_latents(ss, sc, ts, n, m, S, Cn)
    _relclose(zs, torch.cat([src, T64(sc)[:, :Cn]], dim=-1).numpy(), "z_src")
    _relclose(zc, torch.cat([trg, T64(sc)[:, :Cn]], dim=-1).numpy(), "z_conv")
    a, b, c = rs.uniform(0.1, 1, 50), rs.uniform(0.1, 1, 50), rs.uniform(0.1, 1, 50)
    _relclose(E.mul_div(a, b, c), np.multiply(a, np.divide(b, c)), "mul_div")


def test_move_references_against_torch_layout_operations():
    rs = np.random.RandomState(6)
    Bh, C, T = 2, 5, 7
    x1, x2 = rs.rand(Bh, C, T), rs.rand(Bh, C, T)
    fr = torch.cat((T64(x1), T64(x2)), 0).permute(2, 0, 1)
    assert np.array_equal(E.mel_to_frames(x1, x2, Bh, C, T), fr.numpy())
    assert np.array_equal(E.mel_to_frames(x1, None, Bh, C, T), T64(x1).permute(2, 0, 1).numpy())
    assert np.array_equal(E.frames_to_mel(fr.contiguous().numpy(), 2 * Bh, C, T), np.concatenate([x1, x2]))
    W = np.float32(rs.rand(3, 4, 5))
    assert np.array_equal(E.conv_pack_w(W, 3, 4), T64(W).permute(2, 0, 1).numpy())
    assert np.array_equal(E.conv_pack_wt(W, 3, 4), T64(W).permute(2, 1, 0).numpy())
    assert np.array_equal(E.conv_unpack_add_w(E.conv_pack_w(W, 3, 4), np.ones((3, 4, 5)), 3, 4), W + np.float32(1))
    for L in (0, 6, 7, 19):                                  # chunking_mel with 64 -> 7
        mel = rs.rand(C, max(L, 1))[:, :L]
        n = L // T + 1
        data = [mel[:, i * T:i * T + T] if i < n - 1 else np.pad(mel[:, i * T:], ((0, 0), (0, T - L % T))) for i in range(n)]
        ch = E.mel_to_chunks(mel, C, L, T)
        assert np.array_equal(ch, np.stack(data))
        cat = torch.cat([T64(ch)[i] for i in range(n)], 1)
        assert np.array_equal(E.chunks_to_mel(ch, n, C, T, 0.0, 1.0, 0), cat.numpy())
        assert np.array_equal(E.chunks_to_mel(ch, n, C, T, 0.25, 0.5, 1), torch.clamp(cat, min=0.25, max=0.5).numpy())
    mels, lens = rs.rand(3, C, 20), [20, 9, 3]
    out = E.gather_crop(mels, lens, [1, 1, 2, 0], [0, 5, 3, 13], C, T, 20)
    for i, (u, o) in enumerate(zip([1, 1, 2, 0], [0, 5, 3, 13])):
        crop = mels[u][:, :lens[u]][:, o:o + T]
        assert np.array_equal(out[i], np.pad(crop, ((0, 0), (0, T - crop.shape[1]))))


# ------------------------------------------------------------------ 2. the bounds hold on the fp32 restatement
@pytest.mark.parametrize("name", list(E.CASES["latent"]))
def test_latent_bounds_on_the_fp32_restatement(name):
    Bh, S, Cn = E.CASES["latent"][name]
    d = E.latent_inputs(Bh, S, Cn, 20 + Bh)
    worst = {}
    for eps_c in (d["eps_c"], None):
        fb = E.latent_fwd_bounds(d["style"], d["content"], eps_c, d["eps_s"], Bh, S, Cn)
        for up, keys in UPSTREAM.items():
            ups = [d[k] if k in keys else None for k in UPSTREAM["all"]]
            bb = E.latent_bwd_bounds(d["style"], d["content"], eps_c, d["eps_s"], *ups, Bh, S, Cn)
            for push in PUSHES:
                ex = E.exp32(push)
                z = E.latent_fwd(d["style"], d["content"], eps_c, d["eps_s"], Bh, S, Cn, E.F32, ex)[0]
                worst["z"] = max(worst.get("z", 0), _inside(z, fb["z"], fb["tol_z"], "z"))
                ds, dc = E.latent_bwd(d["style"], d["content"], eps_c, d["eps_s"], *ups, Bh, S, Cn, E.F32, ex)
                worst["dstyle"] = max(worst.get("dstyle", 0), _inside(ds, bb["dstyle"], bb["tol_dstyle"], "dstyle " + up))
                worst["dcontent"] = max(worst.get("dcontent", 0), _inside(dc, bb["dcontent"], bb["tol_dcontent"], "dcontent " + up))
                assert not ds[Bh:].view(np.int32).any()
        if eps_c is None:
            assert np.array_equal(fb["z"][:, S:], fb["q_mu"][:, S:]) and (fb["tol_z"][:, S:] == E.FLOOR).all()
    print(f"latent {name}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    # the seeded wrong restatement: the style gradient not halved (and halved twice)
    ups = [d[k] for k in UPSTREAM["all"]]
    bb = E.latent_bwd_bounds(d["style"], d["content"], d["eps_c"], d["eps_s"], *ups, Bh, S, Cn)
    for wrong in (1.0, 0.25):
        ds, _ = E.latent_bwd(d["style"], d["content"], d["eps_c"], d["eps_s"], *ups, Bh, S, Cn, E.F32, E.exp32(0), style_half=wrong)
        assert _outside(ds, bb["dstyle"], bb["tol_dstyle"])


@pytest.mark.parametrize("wide", [True, False])
@pytest.mark.parametrize("n", E.CASES["kl"])
def test_kl_bounds_on_the_fp32_restatement(n, wide):
    rs = np.random.RandomState(n)
    mu, lv = E.edge_mu(rs, n), E.edge_lv(rs, n, wide)
    for scale in (np.float32(-0.5 / 5), np.float32(1.0 / 7)):
        ref, tol = E.kl_fwd_bounds(mu, lv, scale)
        kb = E.kl_bwd_bounds(mu, lv, np.float32(1.7), scale)
        for push in PUSHES:
            ex = E.exp32(push)
            _inside(E.kl_fwd(mu, lv, scale, E.F32, ex), ref, tol, "kl_fwd")
            dmu, dlv = E.kl_bwd(mu, lv, np.float32(1.7), scale, E.F32, ex)
            _inside(dmu, kb["dmu"], kb["tol_dmu"], "dmu")
            _inside(dlv, kb["dlv"], kb["tol_dlv"], "dlv")
        # the seeded wrong restatement: the 1 dropped from 1 - exp(lv) / from the term
        G = np.float32(1.7) * scale
        assert _outside(G * -E.exp32(0)(lv), kb["dlv"], kb["tol_dlv"])
        if not wide:
            wrong = np.float32(E.kl_terms(mu, lv, E.F32, E.exp32(0), drop_one=True).astype(np.float64).sum() * float(scale))
            assert _outside(wrong, ref, tol)


@pytest.mark.parametrize("n", E.CASES["l1"])
def test_l1_bounds_on_the_fp32_restatement(n):
    rs = np.random.RandomState(n % 1000)
    x, y = E.edge_pair(rs, n)
    scale = np.float32(1.0 / 7)
    ref, tol = E.l1_fwd_bounds(x, y, scale)
    _inside(E.l1_fwd_f32(x, y, scale), ref, tol, "l1")
    xe, ye = E.int_pair(rs, n)
    assert float(E.l1_fwd_f32(xe, ye, np.float32(1 / 64))) == E.l1_fwd(xe, ye, np.float32(1 / 64))        # class E is exact
    if n & 3:                                       # the seeded wrong restatement: one tail element skipped
        if n < 2000:
            assert _outside(E.l1_fwd_f32(x, y, scale, skip_tail=1), ref, tol)
        xe[n - 1], ye[n - 1] = 4, -4
        assert float(E.l1_fwd_f32(xe, ye, np.float32(1 / 64), skip_tail=1)) != E.l1_fwd(xe, ye, np.float32(1 / 64))


@pytest.mark.parametrize("wide", [True, False])
@pytest.mark.parametrize("nq,ns", E.CASES["loss_nq_ns"])
@pytest.mark.parametrize("n", [5, 1023])
def test_loss_bounds_on_the_fp32_restatement(n, nq, ns, wide):
    d = E.loss_inputs(n, nq, ns, "R", n + nq, wide)
    for push in PUSHES:
        ex = E.exp32(push)
        out = E.loss_fwd_f32(d, ex)
        ref, tol = E.loss_fwd_bounds(d, out)
        for k in range(8):
            _inside(out[k], ref[k], tol[k], f"out[{k}]")
        for name, g8 in E.G8.items():
            refs, tols = E.loss_bwd_bounds(d, g8)
            got = E.loss_bwd(d, g8, E.F32, ex)
            w32 = E.loss_weights(d, g8, E.F32)[0]
            for k in range(4):
                assert np.array_equal(np.abs(got[k][got[k] != 0]), np.full((got[k] != 0).sum(), abs(w32[k]), np.float32))
                assert np.array_equal(np.sign(got[k]), np.sign(refs[k])) and abs(float(w32[k]) - np.abs(refs[k]).max()) <= tols[k]
            for k in range(4, 10):
                _inside(got[k], refs[k], tols[k], f"{E.LOSS_KEYS[2 + k]} {name}")
    # the seeded wrong restatements: kl_scale and style_scale swapped, one tail element skipped, a tie that gives -w
    ref, tol = E.loss_fwd_bounds(d)
    sw = E.loss_fwd_f32(d, E.exp32(0), swap_scales=True)
    assert ns == 1 or abs(sw[7] - ref[7]) > tol[7]           # (one element: mu = lv = 0, the term is 0 at any scale)
    assert wide or nq == 1 or abs(sw[5] - ref[5]) > tol[5]
    st = E.loss_fwd_f32(d, E.exp32(0), skip_tail=1)
    assert all(abs(st[k] - ref[k]) > tol[k] for k in (1, 2, 3, 4))
    refs, _ = E.loss_bwd_bounds(d, E.G8["ones"])
    bad = E.loss_bwd(d, E.G8["ones"], E.F32, E.exp32(0), tie=-1.0)
    assert not np.array_equal(np.sign(bad[0]), np.sign(refs[0]))


@pytest.mark.parametrize("R,C", [(1, 1), (3, 80), (511, 3), (513, 258), (1025, 520), (8192, 512)])
def test_colsum_bounds_on_the_fp32_restatement(R, C):
    ld = (C + 3) // 4 * 4 + 4
    Xm, old = E.colsum_inputs(R, C, ld, False, "R", R + C), np.float32(np.random.RandomState(1).uniform(-2, 2, C))
    ref, tol = E.colsum_bounds(Xm, C, old)
    _inside(E.colsum_ws_f32(Xm, C, old), ref, tol, "colsum")
    Xe = E.colsum_inputs(R, C, ld, True, "E", R + C)
    assert np.array_equal(E.colsum_ws_f32(Xe, C, old * 0).astype(np.float64), E.colsum(Xe, C))            # class E is exact
    if R % 4 and C % 4 == 0:                         # the seeded wrong restatement: a row lane's count without the + 3
        assert _outside(E.colsum_ws_f32(Xm, C, old, lose_rows=True), ref, tol)
        assert not np.array_equal(E.colsum_ws_f32(Xe, C, old * 0, lose_rows=True).astype(np.float64), E.colsum(Xe, C))


def test_slab_order_is_sequential_and_a_slab_added_twice_shows():
    for ns in E.CASES["slab_nslab"]:
        c, _, slabs = E.slab_inputs(64, ns, 72, "E", ns)
        ref = c.astype(np.float64) + sum(s.astype(np.float64) for s in slabs)
        assert np.array_equal(E.slab_sum_f32(c, slabs, E.ACT_NONE, 1).astype(np.float64), ref)                 # class E is exact
        assert np.array_equal(E.slab_sum_f32(c, slabs, E.ACT_RELU, 1).astype(np.float64), np.maximum(ref, 0))
        if E.slab_windows(ns)[1]:
            assert not np.array_equal(E.slab_sum_f32(c, slabs, E.ACT_NONE, 1, skip_window_step=True).astype(np.float64), ref)
    c, _, slabs = E.slab_inputs(64, 3, 64, "R", 1)
    v = E.slab_sum_f32(c, slabs, E.ACT_RELU, 1)
    assert not v[:4].view(np.int32)[:3].any()       # sums of -0.0, 0 and 0: ReLU stores +0.0


def test_division_and_tanh_bounds_on_the_fp32_restatement():
    rs = np.random.RandomState(9)
    for n, m in E.CASES["conversion"]:
        S, Cn = E.MODEL_S, E.MODEL_CN
        ss, sc, ts = (np.float32(rs.uniform(-1, 1, s)) for s in ((n, 2 * S), (n, 2 * Cn), (m, 2 * S)))
        zs, zc, t1, t2 = E.conversion_bounds(ss, sc, ts, n, m, S, Cn)
        a, b = E.conversion_latents(ss, sc, ts, n, m, S, Cn, E.F32)
        _inside(a[:, :S], zs[:, :S], t1, "z_src")
        _inside(b[:, :S], zc[:, :S], t2, "z_conv")
        assert np.array_equal(a[:, S:], sc[:, :Cn]) and np.array_equal(b[:, S:], sc[:, :Cn])
    a, b, c = (np.float32(rs.uniform(0.1, 2, 1000)) for _ in range(3))
    ref, tol = E.mul_div_bounds(a, b, c)
    _inside(E.mul_div(a, b, c, E.F32), ref, tol, "mul_div")
    u, dz = np.float32(rs.uniform(-4, 4, 1000)), np.float32(rs.uniform(-1, 1, 1000))
    z = np.tanh(u.astype(np.float64)).astype(np.float32)
    _inside(z, np.tanh(u.astype(np.float64)), E.tol_tanh(u), "tanh")
    _inside(E.act_bwd_f32(dz, z, E.ACT_TANH), E.act_bwd(dz, z, E.ACT_TANH), E.tol_act_bwd_tanh(dz, z), "act_bwd tanh")


# ------------------------------------------------------------------ 4. every case reaches the path it is named for
def test_cases_reach_their_paths():
    lat = E.CASES["latent"]
    assert lat["one"] == (1, 1, 1) and lat["model"][1:] == (4, 28)
    tot = 2 * lat["two_blocks"][0] * sum(lat["two_blocks"][1:])
    assert 256 < tot <= 260 and (tot + 255) // 256 == 2                       # a second workgroup with a few live threads
    assert [(-(-n // 256)) for n in E.CASES["kl"]] == [1, 1, 1, 2, 17]        # trips of thread 0 of the one workgroup
    la = {n: E.l1_launch(n) for n in E.CASES["l1"]}
    assert [la[n]["tail"] for n in E.CASES["l1"]] == [1, 3, 0, 1, 3, 3, 0, 3, 0, 3]
    assert [la[n]["trips"] for n in E.CASES["l1"]] == [0, 0, 1, 1, 1, 1, 1, 1, 2, 3]
    assert la[1023]["blocks"] == 1 and la[4099]["blocks"] == 5 and la[524288]["blocks"] == E.L1_BLOCKS == 512 and la[5]["blocks"] == 1
    assert 524288 == 4 * 256 * E.L1_BLOCKS                                    # the last size of one trip
    lb = {n: E.l1_launch(n, E.LOSS_BWD_BLOCKS) for n in E.CASES["l1"]}
    assert [lb[n]["trips"] for n in E.CASES["l1"]] == [0, 0, 1, 1, 1, 1, 1, 1, 1, 2] and lb[1048583]["blocks"] == 1024
    assert [(-(-q // 256), -(-s // 256)) for q, s in E.CASES["loss_nq_ns"]] == [(1, 1), (1, 2), (2, 1)]
    cs = {C: E.colsum_launch(512, C) for C in E.CASES["colsum_C"]}
    assert [cs[C]["ragged"] for C in E.CASES["colsum_C"]] == [True, True, False, True, True, False]
    assert [cs[C]["cb"] for C in E.CASES["colsum_C"]] == [1, 1, 1, 1, 2, 3]
    rb = {R: E.colsum_launch(R, 80) for R in E.CASES["colsum_R"]}
    assert all(v["rows_pb"] == 512 for v in rb.values()) and [rb[R]["nb"] for R in E.CASES["colsum_R"]] == [1, 1, 1, 1, 2, 3, 16]
    assert [R % 4 for R in E.CASES["colsum_R"]] == [1, 3, 3, 0, 1, 1, 0]
    big = E.colsum_launch(*E.CASES["colsum_1024"])
    assert big["rows_pb"] == 1024 and big["nb"] == 512 and E.colsum_launch(524287, 8)["rows_pb"] == 512
    xcd = E.colsum_launch(*E.CASES["colsum_xcd"])
    assert xcd["nb"] == 16 and xcd["cb"] == 2
    assert E.colsum_launch(8192, 512, deterministic=True)["nb"] == 1
    assert [E.slab_windows(k) for k in E.CASES["slab_nslab"]] == [(0, 0, 0), (0, 0, 1), (0, 0, 3), (0, 1, 0), (0, 1, 3), (1, 0, 0),
                                                                   (1, 0, 1), (1, 1, 0), (1, 1, 1), (2, 0, 1)]
    tab = E.fold_table()
    assert len(tab) == 70 and E.fold_launches(len(tab)) == 2 and E.SLAB_FOLD_MAX == 64
    assert min(t[0] for t in tab) == 4 and all(t[0] % 4 == 0 and t[2] % 4 == 0 for t in tab) and len({t[0] for t in tab}) > 30
    assert {E.slab_windows(t[1]) for t in tab} >= {(0, 0, 1), (0, 1, 0), (1, 0, 0), (1, 1, 1), (2, 0, 1)}
    assert [E.nblk(n) for n in E.CASES["act"]] == [1, 2, 2048] and 524293 > 2048 * 256       # the grid-stride loop wraps
    assert [(-(-C // 32), -(-T // 32)) for _, C, T in E.CASES["frames"]] == [(1, 1), (2, 3), (3, 1), (3, 1), (3, 2)]
    assert sorted(c for _, _, c in E.CASES["permute"]) == [4, 8, 132] and any(a == 1 for a, _, _ in E.CASES["permute"]) \
        and any(b == 1 for _, b, _ in E.CASES["permute"])
    assert [(-(-c // 32), -(-r // 32)) for r, c in E.CASES["transpose"]] == [(1, 1), (2, 1), (9, 4), (32, 1)]      # 32 x 32 tiles
    assert [E.nblk(co * ci) for co, ci in E.CASES["conv_pack"]] == [1, 4, 160, 160]                                  # one thread per (co, ci)
    assert [(-(-ci // 32), -(-co // 32)) for co, ci in E.CASES["conv_pack"]] == [(1, 1), (1, 2), (16, 3), (3, 16)]   # conv_pack_wt tiles
    assert E.CASES["conversion"] == [(1, 1), (7, 3)] and [E.nblk(n) for n in E.CASES["mul_div"]] == [1, 4]
    assert 1.0 < E.EXPF_MEASURED < 4.0 and E.EXPF_ROUNDINGS == 2 * E.EXPF_MEASURED
