"""The latent, loss, reduction, activation and layout kernels of csrc/elem.hip on the MI355X through the C ABI, against the
float64 reference of tests/elem_ref.py, element by element.

Every comparison is ONE launch judged from its own inputs.  What elem_ref derives as bit-exact is compared bit for bit (the
style mean / logvar, the copies, every move, the slab sums, ReLU, the L1 gradient's pattern), everything else within the
rounding bounds derived there (eps32 = 2^-24; the device's expf within EXPF_ROUNDINGS of them), at 100 % of the elements,
never a fraction of a tensor's maximum.  Two input classes: E (small integers / powers of two: every sum is exact, the result
must match bit for bit, a lost or doubled term changes the integer) and R (full significands with the edges mixed in:
log-variances over [-30, 30], lv and mu at exactly 0, half-ulp neighbours of 0, x == recon ties, differences of one ulp,
a denormal difference, -0.0).  No NaN or Inf goes into an arithmetic kernel.

Every buffer a launch may write is a guarded one of tests/kernel_harness.py; every padding region an entry point must not
read holds NaN.  The worst error / bound per kernel and quantity over the module is printed at its end.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import assert_same_bits, Buf, EINVAL, F32, F64, guards, L, ok, P, st, Worst
import dvae_amd  # noqa: E402,F401
from dvae_amd import _lib  # noqa: E402
import elem_ref as E  # noqa: E402

ACTS = {"none": E.ACT_NONE, "relu": E.ACT_RELU, "tanh": E.ACT_TANH}
WORST = Worst("test_hip_elem.py", sort=True, ratio_fn=E.worst_ratio)      # kernel / quantity -> worst error / bound
note = WORST.note


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    WORST.report()


# ------------------------------------------------------------------ latent
UPSTREAM = {"all": ("dz", "dq_mu", "dq_lv", "ds_mu", "ds_lv"), "dz_only": ("dz",), "no_dz": ("dq_mu", "dq_lv", "ds_mu", "ds_lv"),
            "no_ds": ("dz", "dq_mu", "dq_lv")}


@pytest.mark.parametrize("with_eps_c", [True, False], ids=["train", "inference"])
@pytest.mark.parametrize("name", list(E.CASES["latent"]))
def test_latent_fwd_and_bwd(name, with_eps_c):
    Bh, S, Cn = E.CASES["latent"][name]
    D = S + Cn
    d = E.latent_inputs(Bh, S, Cn, 20 + Bh)
    b = {k: Buf(None, data=v) for k, v in d.items()}
    eps_c, eps_c_np = (b["eps_c"], d["eps_c"]) if with_eps_c else (None, None)
    z, q_mu, q_lv, s_mu, s_lv = Buf((2 * Bh, D)), Buf((2 * Bh, D)), Buf((2 * Bh, D)), Buf((Bh, S)), Buf((Bh, S))
    ok(L().dvae_latent_fwd(b["style"].ptr, b["content"].ptr, P(eps_c), b["eps_s"].ptr, z.ptr, q_mu.ptr, q_lv.ptr, s_mu.ptr, s_lv.ptr,
                           Bh, S, Cn, st()))
    guards(z, q_mu, q_lv, s_mu, s_lv)
    fb = E.latent_fwd_bounds(d["style"], d["content"], eps_c_np, d["eps_s"], Bh, S, Cn)
    what = f"latent_fwd {name} eps_c={with_eps_c}"
    for buf, key in ((q_mu, "q_mu"), (q_lv, "q_lv"), (s_mu, "s_mu"), (s_lv, "s_lv")):
        assert_same_bits(buf, fb[key], f"{what} {key}")
    note("latent_fwd z", z.np(), fb["z"], fb["tol_z"], what)
    if not with_eps_c:
        assert_same_bits(z.np()[:, S:], d["content"][:, :Cn], what + " z = mu")
    for up, keys in UPSTREAM.items():
        ups = [b[k] if k in keys else None for k in UPSTREAM["all"]]
        ups_np = [d[k] if k in keys else None for k in UPSTREAM["all"]]
        ds, dc = Buf((2 * Bh, 2 * S)), Buf((2 * Bh, 2 * Cn))
        ok(L().dvae_latent_bwd(b["style"].ptr, b["content"].ptr, P(eps_c), b["eps_s"].ptr, *[P(u) for u in ups], ds.ptr, dc.ptr,
                               Bh, S, Cn, st()))
        guards(ds, dc)
        bb = E.latent_bwd_bounds(d["style"], d["content"], eps_c_np, d["eps_s"], *ups_np, Bh, S, Cn)
        note("latent_bwd dstyle", ds.np(), bb["dstyle"], bb["tol_dstyle"], f"{what} {up}")
        note("latent_bwd dcontent", dc.np(), bb["dcontent"], bb["tol_dcontent"], f"{what} {up}")
        assert not ds.bits()[Bh:].any(), "dstyle of the detached x2 rows is not +0.0"


# ------------------------------------------------------------------ KL
@pytest.mark.parametrize("wide", [True, False], ids=["wide", "narrow"])
@pytest.mark.parametrize("n", E.CASES["kl"])
def test_kl_fwd_and_bwd(n, wide):
    rs = np.random.RandomState(n)
    mu, lv = E.edge_mu(rs, n), E.edge_lv(rs, n, wide)
    bmu, blv, gout = Buf(None, data=mu), Buf(None, data=lv), Buf(None, data=F32([1.7]))
    for scale in (F32(-0.5 / 5), F32(1.0 / 7)):
        out, dmu, dlv = Buf((1,)), Buf((n,)), Buf((n,))
        ok(L().dvae_kl_fwd(bmu.ptr, blv.ptr, out.ptr, n, float(scale), st()))
        ok(L().dvae_kl_bwd(bmu.ptr, blv.ptr, gout.ptr, dmu.ptr, dlv.ptr, n, float(scale), st()))
        guards(out, dmu, dlv)
        ref, tol = E.kl_fwd_bounds(mu, lv, scale)
        kb = E.kl_bwd_bounds(mu, lv, F32(1.7), scale)
        what = f"kl n={n} scale={scale} wide={wide}"
        note("kl_fwd" + (" wide" if wide else ""), out.np()[0], ref, tol, what)
        note("kl_bwd dmu", dmu.np(), kb["dmu"], kb["tol_dmu"], what)
        note("kl_bwd dlv", dlv.np(), kb["dlv"], kb["tol_dlv"], what)


# ------------------------------------------------------------------ L1
def l1_ws():
    return Buf((L().dvae_l1_ws_bytes(1),), torch.uint8)


def l1_sum(bx, by, n, scale):
    out, ws = Buf((1,)), l1_ws()
    ok(L().dvae_l1_sum_fwd(bx.ptr, by.ptr, out.ptr, ws.ptr, n, float(scale), st()))
    guards(out, ws)
    return out


@pytest.mark.parametrize("n", E.CASES["l1"])
def test_l1_sum_fwd_and_bwd(n):
    rs = np.random.RandomState(n % 1000)
    x, y = E.edge_pair(rs, n)
    scale, gv = F32(1.0 / 7), F32(1.3)
    bx, by, gout = Buf(None, data=x), Buf(None, data=y), Buf(None, data=F32([gv]))
    ref, tol = E.l1_fwd_bounds(x, y, scale)
    note("l1_sum_fwd", l1_sum(bx, by, n, scale).np()[0], ref, tol, f"l1 n={n}")
    dy = Buf((n,))
    ok(L().dvae_l1_sum_bwd(bx.ptr, by.ptr, gout.ptr, dy.ptr, n, float(scale), st()))
    guards(dy)
    assert_same_bits(dy, E.l1_bwd(x, y, gv, scale, F32), f"l1_bwd n={n}")            # one product, then a select: exact
    xe, ye = E.int_pair(rs, n)
    xe[n - 1], ye[n - 1] = 4, -4
    bxe, bye = Buf(None, data=xe), Buf(None, data=ye)
    oe = l1_sum(bxe, bye, n, F32(1 / 64))
    assert_same_bits(oe, F32([E.l1_fwd(xe, ye, F32(1 / 64))]), f"l1 class E n={n}")


# ------------------------------------------------------------------ the fused loss
def loss_desc(b, d):
    desc = _lib.LossDesc()
    for k in E.LOSS_KEYS:
        setattr(desc, k, b[k] if isinstance(b[k], int) else b[k].ptr)
    desc.n, desc.nq, desc.ns = d["n"], d["nq"], d["ns"]
    for k in E.SCALE_KEYS:
        setattr(desc, k, float(d[k]))
    return desc


def loss_fwd(desc):
    out, ws = Buf((8,)), Buf((L().dvae_loss_ws_bytes(1),), torch.uint8)
    ok(L().dvae_loss_fwd(ctypes.byref(desc), out.ptr, ws.ptr, st()))
    guards(out, ws)
    return out


def loss_bwd(desc, d, g8, null=()):
    """The ten gradient buffers (None where `null` names them) after one dvae_loss_bwd."""
    n, nq, ns = d["n"], d["nq"], d["ns"]
    outs = [None if k in null else Buf((m,)) for k, m in zip(range(10), (n, n, n, n, nq, nq, nq, nq, ns, ns))]
    ok(L().dvae_loss_bwd(ctypes.byref(desc), g8.ptr, *[P(o) for o in outs], st()))
    guards(*outs)
    return outs


def check_d_recon(buf, x, r, wref, tolw, what, key):
    got, sref = buf.np(), -np.sign(np.asarray(x, F64) - np.asarray(r, F64))
    nz = got != 0
    assert np.array_equal(nz, sref != 0), f"{what}: zero exactly at the ties"
    assert not buf.bits()[~nz].any(), f"{what}: a tie is not +0.0"
    if nz.any():
        i = int(np.argmax(nz))
        w = F32(got[i] * sref[i])
        assert np.array_equal(got[nz], (sref[nz] * w).astype(F32)), f"{what}: more than one weight, or a wrong sign"
        note(key, w, wref, tolw, what)


LOSS_SHAPES = list(zip(E.CASES["l1"], [E.CASES["loss_nq_ns"][i % 3] for i in range(len(E.CASES["l1"]))]))


@pytest.mark.parametrize("n,nqs", LOSS_SHAPES, ids=[str(n) for n, _ in LOSS_SHAPES])
def test_loss_fwd_and_bwd(n, nqs):
    nq, ns = nqs
    for wide in ((True, False) if n <= 4099 else (n % 2 == 0,)):
        d = E.loss_inputs(n, nq, ns, "R", n % 1000 + nq, wide)
        b = {k: Buf(None, data=d[k]) for k in E.LOSS_KEYS}
        desc = loss_desc(b, d)
        out = loss_fwd(desc)
        o = out.np()
        what = f"loss n={n} nq={nq} ns={ns} wide={wide}"
        ref, tol = E.loss_fwd_bounds(d, o)
        for k, nm in enumerate(("total", "l1", "l1", "l1", "l1", "kl", "kl", "kl_style")):
            note("loss_fwd " + nm + (" wide" if wide and k > 4 else ""), o[k], ref[k], tol[k], f"{what} out[{k}]")
        for k in range(4):                    # the same block count and order as dvae_l1_sum_fwd: the same bits
            alone = l1_sum(b["x%d" % (1 + (k & 1))], b[E.LOSS_KEYS[2 + k]], n, d["l1_scale"])
            assert alone.bits()[0] == out.bits()[1 + k], f"{what}: out[{1 + k}] is not dvae_l1_sum_fwd's"
        for gname, g8 in E.G8.items():
            if n > 4099 and gname != "random":
                continue
            outs = loss_bwd(desc, d, Buf(None, data=g8))
            refs, tols = E.loss_bwd_bounds(d, g8)
            wref = E.loss_weights(d, g8.astype(F64))[0]
            for k in range(4):
                check_d_recon(outs[k], d["x%d" % (1 + (k & 1))], d[E.LOSS_KEYS[2 + k]], wref[k], tols[k], f"{what} {gname} d_recon {k}", "loss_bwd w")
            for k in range(4, 10):
                note("loss_bwd d" + ("mu" if k % 2 == 0 else "lv"), outs[k].np(), refs[k], tols[k], f"{what} {gname} {E.LOSS_KEYS[2 + k]}")


@pytest.mark.parametrize("n", [5, 1023, 1048583])
def test_loss_bwd_null_outputs_leave_the_others_their_bits(n):
    nq, ns = 257, 300
    d = E.loss_inputs(n, nq, ns, "R", 77)
    b = {k: Buf(None, data=d[k]) for k in E.LOSS_KEYS}
    desc, g8 = loss_desc(b, d), Buf(None, data=E.G8["random"])
    full = [o.bits() for o in loss_bwd(desc, d, g8)]
    for null in ((0,), (1,), (2,), (3,), (4, 5), (6, 7), (8, 9), (0, 1, 2, 3), (4, 5, 6, 7, 8, 9)):
        if n > 5000 and len(null) == 1 and null[0] not in (0, 3):
            continue
        outs = loss_bwd(desc, d, g8, null)
        for k in range(10):
            assert (outs[k] is None) == (k in null)
            assert outs[k] is None or np.array_equal(outs[k].bits(), full[k]), f"null {null}: output {k} changed"


def test_loss_on_the_halves_of_one_tensor_as_pointer_offsets():
    """What ops.LossGVAE2FullFn passes: recon1 | recon2 and the q halves are offsets into one buffer; the gradients too."""
    n, nq, ns = 4100, 160, 20
    d = E.loss_inputs(n, nq, ns, "R", 5)
    b = {k: Buf(None, data=d[k]) for k in E.LOSS_KEYS}
    sep_out = loss_fwd(loss_desc(b, d)).bits()
    g8 = Buf(None, data=E.G8["random"])
    sep = [o.bits() for o in loss_bwd(loss_desc(b, d), d, g8)]
    cat = lambda a, c: Buf(None, data=np.concatenate([d[a], d[c]]))
    rec, hat, qmu, qlv = cat("recon1", "recon2"), cat("recon1_hat", "recon2_hat"), cat("q1_mu", "q2_mu"), cat("q1_lv", "q2_lv")
    pb = dict(b, recon1=rec.ptr, recon2=rec.ptr + 4 * n, recon1_hat=hat.ptr, recon2_hat=hat.ptr + 4 * n, q1_mu=qmu.ptr,
              q2_mu=qmu.ptr + 4 * nq, q1_lv=qlv.ptr, q2_lv=qlv.ptr + 4 * nq)
    desc = loss_desc(pb, d)
    assert np.array_equal(loss_fwd(desc).bits(), sep_out)
    grec, ghat, gmu, glv, gsm, gsl = Buf((2 * n,)), Buf((2 * n,)), Buf((2 * nq,)), Buf((2 * nq,)), Buf((ns,)), Buf((ns,))
    ok(L().dvae_loss_bwd(ctypes.byref(desc), g8.ptr, grec.ptr, grec.ptr + 4 * n, ghat.ptr, ghat.ptr + 4 * n, gmu.ptr, glv.ptr,
                         gmu.ptr + 4 * nq, glv.ptr + 4 * nq, gsm.ptr, gsl.ptr, st()))
    guards(grec, ghat, gmu, glv, gsm, gsl)
    for got, k1, k2 in ((grec, 0, 1), (ghat, 2, 3), (gmu, 4, 6), (glv, 5, 7)):
        assert np.array_equal(got.bits(), np.concatenate([sep[k1], sep[k2]]))
    assert np.array_equal(gsm.bits(), sep[8]) and np.array_equal(gsl.bits(), sep[9])


@pytest.mark.parametrize("n", [5, 524291, 1048583])
def test_loss_l1_entries_are_exact_on_integers(n):
    d = E.loss_inputs(n, 1, 1, "E", n % 1000)
    b = {k: Buf(None, data=d[k]) for k in E.LOSS_KEYS}
    o = loss_fwd(loss_desc(b, d))
    assert_same_bits(o.np()[1:5], F32(E.loss_fwd(d)[1:5]), f"loss class E n={n}")


# ------------------------------------------------------------------ column sums
def colsum_call(variant, Xb, o1, o2, R, C, ld, b16, ws):
    if variant == "ws":
        return L().dvae_colsum_add_ws(Xb.ptr, o1.ptr, P(o2), R, C, ld, int(b16), ws.ptr, st())
    return L().dvae_colsum_add(Xb.ptr, o1.ptr, P(o2), R, C, ld, int(b16), st())


def colsum_case(variant, R, C, ld, b16, cls, with_o2, seed):
    Xm = E.colsum_inputs(R, C, ld, b16, cls, seed)
    rs = np.random.RandomState(seed + 1)
    old1 = F32(rs.randint(-8, 9, C)) if cls == "E" else F32(rs.uniform(-2, 2, C))
    old2 = F32(np.zeros(C))
    Xb = Buf(None, torch.bfloat16 if b16 else torch.float32, data=Xm)
    what = f"colsum {variant} R={R} C={C} ld={ld} bf16={b16} class {cls}"
    ws, first = None, None
    if variant == "ws":
        nbytes = L().dvae_colsum_ws_bytes(R, C)
        la = E.colsum_launch(R, C)
        assert nbytes == 4096 + la["nb"] * la["cb"] * 256 * 4
        ws = Buf((nbytes,), torch.uint8)                      # the partial sums start as NaN ...
        ws.t[:4096].zero_()                                   # ... the counters as the contract says
    for call in range(2 if variant == "ws" else 1):
        o1, o2 = Buf(None, data=old1), (Buf(None, data=old2) if with_o2 else None)
        ok(colsum_call(variant, Xb, o1, o2, R, C, ld, b16, ws))
        guards(o1, o2, ws)
        if ws is not None:
            assert not ws.bits()[:4096].any(), f"{what}: the counters are not left zero"
        for o, old in ((o1, old1), (o2, old2)):
            if o is None:
                continue
            if cls == "E":
                assert_same_bits(o, F32(E.colsum(Xm, C, old)), what)
            else:
                ref, tol = E.colsum_bounds(Xm, C, old, variant)
                note(f"colsum {variant}" + (" bf16" if b16 else ""), o.np(), ref, tol, what)
        if first is not None:
            assert np.array_equal(first, o1.bits()), f"{what}: the second call on the same workspace differs"
        first = o1.bits()


@pytest.mark.parametrize("variant", ["ws", "atomic", "deterministic"])
@pytest.mark.parametrize("R", E.CASES["colsum_R"])
def test_colsum(R, variant):
    was = L().dvae_get_deterministic()
    try:
        L().dvae_set_deterministic(1 if variant == "deterministic" else 0)
        k = 0
        for C in E.CASES["colsum_C"]:
            for b16 in (False, True):
                for ld in ((C + 3) // 4 * 4, (C + 3) // 4 * 4 + 8):
                    k += 1
                    for cls in (("R", "E") if R <= 1025 else ("RE"[(k + k // 2) % 2],)):
                        colsum_case(variant, R, C, ld, b16, cls, k % 3 != 0, 1000 * R + C)      # (out2 null for every third shape)
    finally:
        L().dvae_set_deterministic(was)


@pytest.mark.parametrize("variant", ["ws", "atomic"])
@pytest.mark.parametrize("shape", ["colsum_1024", "colsum_xcd"])
def test_colsum_many_row_blocks(shape, variant):
    """524288 x 8 in bf16: the 1024-row variant, 512 row blocks.  8192 x 512: 16 row blocks per column block on several
    XCDs, in class E: a stale partial sum is an integer mismatch or a NaN."""
    R, C = E.CASES[shape]
    assert L().dvae_get_deterministic() == 0
    for cls in ("E", "R"):
        colsum_case(variant, R, C, C + 8, shape == "colsum_1024", cls, True, 3)
        if shape == "colsum_xcd":
            colsum_case(variant, R, C, C, False, cls, False, 4)


# ------------------------------------------------------------------ slab sums
def slab_case(n, nslab, stride, act, accumulate, cls, seed):
    c, store, slabs = E.slab_inputs(n, nslab, stride, cls, seed)
    cb = Buf(None, data=c) if accumulate else Buf((n,))          # accumulate = 0: C holds NaN and must not be read
    sb = Buf(None, data=store)
    ok(L().dvae_slab_sum(cb.ptr, sb.ptr if nslab else None, stride, nslab, n, act, accumulate, st()))
    guards(cb, sb)
    u = E.slab_sum_f32(c, slabs, E.ACT_NONE, accumulate)
    what = f"slab_sum n={n} nslab={nslab} stride={stride} act={act} accumulate={accumulate} class {cls}"
    if act == E.ACT_TANH:
        note("slab_sum tanh", cb.np(), np.tanh(u.astype(F64)), E.tol_tanh(u), what)
    else:
        assert_same_bits(cb, E.slab_sum_f32(c, slabs, act, accumulate), what)
    if cls == "E" and act == E.ACT_NONE:                            # ... and the sequential sum is the exact one
        exact = (c.astype(F64) if accumulate else 0.0) + sum(s.astype(F64) for s in slabs)
        assert np.array_equal(cb.np().astype(F64), exact), what


@pytest.mark.parametrize("nslab", E.CASES["slab_nslab"])
def test_slab_sum(nslab):
    n = 2060                                                          # three workgroups, the last one partly idle
    for act in ACTS.values():
        for accumulate in (0, 1):
            if nslab == 0 and not accumulate:
                continue                                              # refused (test_refusals)
            for stride in (n, n + 8):
                for cls in ("E", "R"):
                    slab_case(n, nslab, stride, act, accumulate, cls, 10 * nslab + act)
    if nslab in (1, 9):
        slab_case(4, nslab, 4, E.ACT_RELU, 0, "R", 3)
    if nslab == 1:                                                    # n4 > 2048 * 256: the grid-stride loop wraps
        n = 4 * (2048 * 256 + 5)
        assert E.nblk(n // 4, 256, 2048) * 256 < n // 4
        slab_case(n, 1, n, E.ACT_RELU, 1, "R", 4)


def test_slab_fold_seventy_entries():
    tab = E.fold_table()
    for cls in ("E", "R"):
        descs, keep, want = (_lib.SlabDesc * len(tab))(), [], []
        for e, (n, nslab, stride, seed) in enumerate(tab):
            c, store, slabs = E.slab_inputs(n, nslab, stride, cls, seed)
            cb, sb = Buf(None, data=c), Buf(None, data=store)
            keep.append((cb, sb))
            want.append(E.slab_sum_f32(c, slabs, E.ACT_NONE, 1))
            descs[e].c, descs[e].slab, descs[e].slab_stride, descs[e].n, descs[e].nslab = cb.ptr, sb.ptr, stride, n, nslab
        ok(L().dvae_slab_fold(descs, len(tab), st()))
        for e, (cb, sb) in enumerate(keep):
            guards(cb, sb)
            assert_same_bits(cb, want[e], f"slab_fold class {cls} entry {e} {tab[e][:3]}")


# ------------------------------------------------------------------ activations
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("n", E.CASES["act"])
def test_act_fwd_and_bwd(n, act):
    a = ACTS[act]
    rs = np.random.RandomState(n % 1000 + a)
    u, dz = F32(rs.uniform(-6, 6, n)), F32(rs.uniform(-1, 1, n))
    u[::5] = F32(rs.uniform(-1e-3, 1e-3, len(u[::5])))
    u[0] = -0.0
    if n > 4:
        u[1:5], dz[1:5] = [0.0, -2.0 ** -149, 2.0 ** -149, -0.0], [-1.0, 1.0, -0.0, -0.5]
    y = Buf(None, data=u)
    ok(L().dvae_act_fwd(y.ptr, n, a, st()))
    guards(y)
    what = f"act n={n} {act}"
    if a == E.ACT_TANH:
        note("act_fwd tanh", y.np(), np.tanh(u.astype(F64)), E.tol_tanh(u), what)
    else:
        assert_same_bits(y, np.where(u > 0, u, F32(0)) if a == E.ACT_RELU else u, what + " forward")
    z = y.np()
    zb, dzb, du = Buf(None, data=z), Buf(None, data=dz), Buf((n,))
    ok(L().dvae_act_bwd(dzb.ptr, zb.ptr, du.ptr, n, a, st()))
    guards(du)
    if a == E.ACT_TANH:
        note("act_bwd tanh", du.np(), E.act_bwd(dz, z, a), E.tol_act_bwd_tanh(dz, z), what)
    else:
        assert_same_bits(du, E.act_bwd_f32(dz, z, a), what + " backward")
    ok(L().dvae_act_bwd(dzb.ptr, zb.ptr, dzb.ptr, n, a, st()))          # dU may alias dZ
    guards(dzb)
    assert np.array_equal(dzb.bits(), du.bits())


# ------------------------------------------------------------------ moves: int32 bit patterns of random bits
def rbits(rs, *shape):
    return rs.randint(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32).view(F32)


@pytest.mark.parametrize("shape", E.CASES["frames"], ids=lambda s: "x".join(map(str, s)))
def test_mel_to_frames_and_back(shape):
    Bh, C, T = shape
    rs = np.random.RandomState(sum(shape))
    x1, x2 = rbits(rs, Bh, C, T), rbits(rs, Bh, C, T)
    b1, b2 = Buf(None, data=x1), Buf(None, data=x2)
    for second in (b2, None):
        N = 2 * Bh if second is not None else Bh
        X = Buf((T, N, C))
        ok(L().dvae_mel_to_frames(b1.ptr, P(second), X.ptr, Bh, C, T, 0, st()))
        guards(X)
        want = E.mel_to_frames(x1, x2 if second is not None else None, Bh, C, T)
        assert_same_bits(X, want, f"mel_to_frames {shape} x2={second is not None}")
        back = Buf((N, C, T))
        ok(L().dvae_frames_to_mel(X.ptr, back.ptr, N, C, T, st()))
        guards(back)
        assert_same_bits(back, np.concatenate([x1, x2]) if second is not None else x1, f"frames_to_mel {shape}")
    # bf16: finite inputs with exact round-to-nearest-even ties; the bits must be torch's .bfloat16()
    f1 = F32(rs.uniform(-4, 4, (Bh, C, T)))
    tie = (f1.view(np.uint32) & np.uint32(0xFFFF0000)) | np.uint32(0x8000)          # exactly half way between two bf16
    f1.reshape(-1)[::3] = tie.view(F32).reshape(-1)[::3]
    f1.reshape(-1)[0] = -0.0
    f2 = F32(rs.uniform(-1e-3, 1e-3, (Bh, C, T)))
    X16 = Buf((T, 2 * Bh, C), torch.bfloat16)
    g1, g2 = Buf(None, data=f1), Buf(None, data=f2)
    ok(L().dvae_mel_to_frames(g1.ptr, g2.ptr, X16.ptr, Bh, C, T, 1, st()))
    guards(X16)
    want = torch.from_numpy(E.mel_to_frames(f1, f2, Bh, C, T)).bfloat16().view(torch.int16).numpy()
    assert np.array_equal(X16.bits(), want), f"mel_to_frames bf16 {shape}: not the round-to-nearest-even bf16"


def test_permute_transpose_and_conv_packs():
    rs = np.random.RandomState(12)
    for A, B_, C in E.CASES["permute"]:
        x = rbits(rs, A, B_, C)
        xb, o = Buf(None, data=x), Buf((B_, A, C))
        ok(L().dvae_permute_102(xb.ptr, o.ptr, A, B_, C, st()))
        guards(o)
        assert_same_bits(o, x.transpose(1, 0, 2), f"permute_102 {A}x{B_}x{C}")
    for R, C in E.CASES["transpose"]:
        x = rbits(rs, R, C)
        xb, o = Buf(None, data=x), Buf((C, R))
        ok(L().dvae_transpose(xb.ptr, o.ptr, R, C, st()))
        guards(o)
        assert_same_bits(o, x.T, f"transpose {R}x{C}")
    for Cout, Cin in E.CASES["conv_pack"]:
        W = rbits(rs, Cout, Cin, 5)
        Wb, p, pt = Buf(None, data=W), Buf((5, Cout, Cin)), Buf((5, Cin, Cout))
        ok(L().dvae_conv_pack_w(Wb.ptr, p.ptr, Cout, Cin, st()))
        ok(L().dvae_conv_pack_wt(Wb.ptr, pt.ptr, Cout, Cin, st()))
        guards(p, pt)
        assert_same_bits(p, E.conv_pack_w(W, Cout, Cin), f"conv_pack_w {Cout}x{Cin}")
        assert_same_bits(pt, E.conv_pack_wt(W, Cout, Cin), f"conv_pack_wt {Cout}x{Cin}")
        dWp, dW = F32(rs.uniform(-1, 1, (5, Cout, Cin))), F32(rs.uniform(-1, 1, (Cout, Cin, 5)))
        dWp.reshape(-1)[:2], dW.reshape(-1)[0] = [-0.0, 3.0], -0.0
        acc, src = Buf(None, data=dW), Buf(None, data=dWp)
        ok(L().dvae_conv_unpack_add_w(src.ptr, acc.ptr, Cout, Cin, st()))
        guards(acc)
        assert_same_bits(acc, E.conv_unpack_add_w(dWp, dW, Cout, Cin), f"conv_unpack_add_w {Cout}x{Cin}")


def test_gather_crop():
    """Repeated utterances; off + T inside, across and beyond lens[u]; Lmax > lens: the columns behind lens[u] hold NaN."""
    rs = np.random.RandomState(13)
    C, T, Lmax = 5, 7, 40
    lens = np.array([40, 9, 3, 25], np.int32)
    mels = rbits(rs, len(lens), C, Lmax)
    for u, l in enumerate(lens):
        mels[u, :, l:] = np.nan
    utt = np.array([1, 1, 2, 0, 3, 0, 1, 2], np.int32)
    off = np.array([0, 5, 0, 33, 18, 34, 9, 3], np.int32)             # inside, across, across, inside (the end), inside (the end), across, beyond, beyond
    out, ins = Buf((len(utt), C, T)), [Buf(None, data=a) for a in (mels, lens, utt, off)]
    ok(L().dvae_gather_crop(*[i.ptr for i in ins], out.ptr, len(utt), C, T, Lmax, st()))
    guards(out)
    assert_same_bits(out, E.gather_crop(mels, lens, utt, off, C, T, Lmax), "gather_crop")


@pytest.mark.parametrize("Lk", ["0", "T-1", "T", "2T+5"])
def test_mel_to_chunks_and_chunks_to_mel(Lk):
    C, T = 5, 8
    Lm = {"0": 0, "T-1": T - 1, "T": T, "2T+5": 2 * T + 5}[Lk]
    rs = np.random.RandomState(Lm)
    mel = rbits(rs, C, Lm)
    n = Lm // T + 1
    melb = Buf(None, data=mel) if Lm else Buf((C, 1))                 # L = 0: nothing may be read
    out = Buf((n, C, T))
    ok(L().dvae_mel_to_chunks(melb.ptr, out.ptr, C, Lm, T, n, st()))
    guards(out)
    assert_same_bits(out, E.mel_to_chunks(mel, C, Lm, T), f"mel_to_chunks L={Lm}")
    lo, hi = F32(0.0), F32(1.0)
    x = F32(rs.uniform(-0.5, 1.5, (n, C, T)))
    x.reshape(-1)[:6] = [lo, hi, np.nextafter(lo, F32(-1)), np.nextafter(hi, F32(2)), np.nextafter(hi, F32(0)), 2.0 ** -149]
    xb = Buf(None, data=x)
    for clamp in (0, 1):
        o = Buf((C, n * T))
        ok(L().dvae_chunks_to_mel(xb.ptr, o.ptr, n, C, T, float(lo), float(hi), clamp, st()))
        guards(o)
        assert_same_bits(o, E.chunks_to_mel(x, n, C, T, lo, hi, clamp), f"chunks_to_mel n={n} clamp={clamp}")
    raw = rbits(rs, n, C, T)                                          # clamp off moves bits
    rb, o = Buf(None, data=raw), Buf((C, n * T))
    ok(L().dvae_chunks_to_mel(rb.ptr, o.ptr, n, C, T, 0.0, 1.0, 0, st()))
    guards(o)
    assert_same_bits(o, E.chunks_to_mel(raw, n, C, T, 0, 1, 0), "chunks_to_mel on random bits")


# ------------------------------------------------------------------ conversion
@pytest.mark.parametrize("n,m", E.CASES["conversion"])
def test_conversion_latents(n, m):
    S, Cn = E.MODEL_S, E.MODEL_CN
    rs = np.random.RandomState(n + m)
    ss, sc, ts = (F32(rs.uniform(-2, 2, s)) for s in ((n, 2 * S), (n, 2 * Cn), (m, 2 * S)))
    ss[:, S:], ts[:, S:], sc[:, Cn:] = np.nan, np.nan, np.nan          # the log-variances are not read
    zs, zc, ins = Buf((n, S + Cn)), Buf((n, S + Cn)), [Buf(None, data=a) for a in (ss, sc, ts)]
    ok(L().dvae_conversion_latents(*[i.ptr for i in ins], zs.ptr, zc.ptr, n, m, S, Cn, st()))
    guards(zs, zc)
    rs_, rc_, t1, t2 = E.conversion_bounds(ss, sc, ts, n, m, S, Cn)
    note("conversion_latents mean", zs.np()[:, :S], rs_[:, :S], t1, f"z_src {n}x{m}")
    note("conversion_latents mean", zc.np()[:, :S], rc_[:, :S], t2, f"z_conv {n}x{m}")
    assert_same_bits(zs.np()[:, S:], sc[:, :Cn], "z_src content")
    assert_same_bits(zc.np()[:, S:], sc[:, :Cn], "z_conv content")


@pytest.mark.parametrize("n", E.CASES["mul_div"])
def test_mul_div(n):
    rs = np.random.RandomState(n)
    a, b, c = (F32(rs.uniform(0.05, 2, n) * rs.choice([-1.0, 1.0], n)) for _ in range(3))
    o, ins = Buf((n,)), [Buf(None, data=v) for v in (a, b, c)]
    ok(L().dvae_mul_div(*[i.ptr for i in ins], o.ptr, n, st()))
    guards(o)
    ref, tol = E.mul_div_bounds(a, b, c)
    note("mul_div", o.np(), ref, tol, f"mul_div n={n}")


# ------------------------------------------------------------------ argument refusals (only what the entry points' code refuses)
def test_refusals_change_nothing():
    lib, s = L(), st()
    x, y, o = Buf(None, data=F32(np.ones(64))), Buf(None, data=F32(np.ones(64))), Buf((64,))
    i32 = Buf(None, data=np.zeros(8, np.int32))
    ws = Buf((16384,), torch.uint8, fill=0)
    before = o.bits()
    p, q, w = x.ptr, y.ptr, o.ptr
    E_ = EINVAL
    assert lib.dvae_latent_fwd(None, p, p, p, w, w, w, w, w, 1, 1, 1, s) == E_
    assert lib.dvae_latent_fwd(p, p, p, None, w, w, w, w, w, 1, 1, 1, s) == E_
    assert lib.dvae_latent_fwd(p, p, p, p, w, w, w, w, None, 1, 1, 1, s) == E_
    for dims in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert lib.dvae_latent_fwd(p, p, p, p, w, w, w, w, w, *dims, s) == E_
        assert lib.dvae_latent_bwd(p, p, p, p, p, p, p, p, p, w, w, *dims, s) == E_
    assert lib.dvae_latent_bwd(p, p, p, None, p, p, p, p, p, w, w, 1, 1, 1, s) == E_
    assert lib.dvae_latent_bwd(p, p, p, p, p, p, p, p, p, None, w, 1, 1, 1, s) == E_
    assert lib.dvae_kl_fwd(p, q, w, 0, 1.0, s) == E_ and lib.dvae_kl_fwd(p, None, w, 4, 1.0, s) == E_
    assert lib.dvae_kl_bwd(p, q, p, w, w, 0, 1.0, s) == E_ and lib.dvae_kl_bwd(p, q, None, w, w, 4, 1.0, s) == E_
    assert lib.dvae_kl_bwd(p, q, p, w, None, 4, 1.0, s) == E_
    assert lib.dvae_l1_sum_fwd(p, q, w, ws.ptr, 0, 1.0, s) == E_ and lib.dvae_l1_sum_fwd(p, q, w, None, 4, 1.0, s) == E_
    assert lib.dvae_l1_sum_fwd(p + 4, q, w, ws.ptr, 4, 1.0, s) == E_ and lib.dvae_l1_sum_fwd(p, q + 8, w, ws.ptr, 4, 1.0, s) == E_
    assert lib.dvae_l1_sum_bwd(p, q, p, w, 0, 1.0, s) == E_ and lib.dvae_l1_sum_bwd(p, q, None, w, 4, 1.0, s) == E_
    d = {k: x for k in E.LOSS_KEYS}
    sc = dict(n=8, nq=4, ns=4, l1_scale=1.0, kl_scale=1.0, style_scale=1.0, mse_cof=1.0, kl_cof=1.0)
    good = loss_desc(d, sc)
    assert lib.dvae_loss_fwd(None, w, ws.ptr, s) == E_
    assert lib.dvae_loss_fwd(ctypes.byref(good), None, ws.ptr, s) == E_ and lib.dvae_loss_fwd(ctypes.byref(good), w, None, s) == E_
    for k, v in (("n", 0), ("nq", 0), ("ns", 0)):
        assert lib.dvae_loss_fwd(ctypes.byref(loss_desc(d, dict(sc, **{k: v}))), w, ws.ptr, s) == E_
    for k in E.LOSS_KEYS:
        bad = loss_desc(d, sc)
        setattr(bad, k, None)
        assert lib.dvae_loss_fwd(ctypes.byref(bad), w, ws.ptr, s) == E_, k
        assert lib.dvae_loss_bwd(ctypes.byref(bad), p, *[w] * 10, s) == E_, k
    for k in E.LOSS_KEYS[:6]:
        assert lib.dvae_loss_fwd(ctypes.byref(loss_desc(dict(d, **{k: p + 4}), sc)), w, ws.ptr, s) == E_, k
    gb = ctypes.byref(good)
    assert lib.dvae_loss_bwd(gb, None, *[w] * 10, s) == E_
    assert lib.dvae_loss_bwd(gb, p, w, w, w, w, w, None, w, w, w, w, s) == E_          # a (mu, lv) pair with one null
    assert lib.dvae_loss_bwd(gb, p, w, w, w, w, w, w, None, w, w, w, s) == E_
    assert lib.dvae_loss_bwd(gb, p, w, w, w, w, w, w, w, w, w, None, s) == E_
    assert lib.dvae_loss_bwd(gb, p, w + 4, w, w, w, w, w, w, w, w, w, s) == E_         # a misaligned d_recon
    for b16 in (0, 1):
        assert lib.dvae_colsum_add(None, w, None, 4, 4, 4, b16, s) == E_ and lib.dvae_colsum_add(p, None, None, 4, 4, 4, b16, s) == E_
        assert lib.dvae_colsum_add(p, w, None, 0, 4, 4, b16, s) == E_ and lib.dvae_colsum_add(p, w, None, 4, 0, 4, b16, s) == E_
        assert lib.dvae_colsum_add(p, w, None, 4, 4, 6, b16, s) == E_
        assert lib.dvae_colsum_add(p + (4 if b16 else 8), w, None, 4, 4, 4, b16, s) == E_
        assert lib.dvae_colsum_add_ws(p, w, None, 4, 4, 4, b16, None, s) == E_ and lib.dvae_colsum_add_ws(p, w, None, 4, 4, 6, b16, ws.ptr, s) == E_
        assert lib.dvae_colsum_add_ws(p, w, None, 4, 4, 4, b16, ws.ptr + 8, s) == E_
        assert lib.dvae_colsum_add_ws(p + (4 if b16 else 8), w, None, 4, 4, 4, b16, ws.ptr, s) == E_
        assert lib.dvae_colsum_add_ws(p, w, None, 1, 256 * 1024 + 1, 256 * 1024 + 4, b16, ws.ptr, s) == E_
        assert lib.dvae_colsum_add_ws(p, w, None, 0, 4, 4, b16, ws.ptr, s) == E_
    assert lib.dvae_colsum_ws_bytes(0, 4) == 0 and lib.dvae_colsum_ws_bytes(4, 0) == 0
    assert lib.dvae_slab_sum(None, p, 8, 1, 8, 0, 1, s) == E_ and lib.dvae_slab_sum(w, p, 8, 1, 0, 0, 1, s) == E_
    assert lib.dvae_slab_sum(w, p, 8, 1, 6, 0, 1, s) == E_ and lib.dvae_slab_sum(w, p, 8, -1, 8, 0, 1, s) == E_
    assert lib.dvae_slab_sum(w, None, 8, 1, 8, 0, 1, s) == E_ and lib.dvae_slab_sum(w, p, 6, 1, 8, 0, 1, s) == E_
    assert lib.dvae_slab_sum(w, p + 4, 8, 1, 8, 0, 1, s) == E_ and lib.dvae_slab_sum(w + 4, p, 8, 1, 8, 0, 1, s) == E_
    assert lib.dvae_slab_sum(w, None, 8, 0, 8, 1, 0, s) == E_                             # nothing to add and nothing to keep
    assert lib.dvae_slab_sum(w, None, 8, 0, 8, 0, 1, s) == 0                              # act none on C alone: nothing to do
    assert lib.dvae_slab_fold(None, 1, s) == E_
    one = (_lib.SlabDesc * 1)()
    for field, v in (("c", None), ("slab", None), ("n", 0), ("n", 6), ("slab_stride", 6), ("nslab", 0), ("c", w + 4), ("slab", p + 8)):
        one[0].c, one[0].slab, one[0].slab_stride, one[0].n, one[0].nslab = w, p, 8, 8, 1
        setattr(one[0], field, v)
        assert lib.dvae_slab_fold(one, 1, s) == E_, field
    assert lib.dvae_slab_fold(one, -1, s) == E_ and lib.dvae_slab_fold(one, 0, s) == 0
    assert lib.dvae_act_fwd(None, 4, 1, s) == E_ and lib.dvae_act_fwd(w, 0, 1, s) == E_
    assert lib.dvae_act_bwd(p, q, None, 4, 1, s) == E_ and lib.dvae_act_bwd(p, q, w, 0, 1, s) == E_
    assert lib.dvae_mel_to_frames(None, p, w, 1, 1, 1, 0, s) == E_ and lib.dvae_mel_to_frames(p, p, None, 1, 1, 1, 0, s) == E_
    for dims in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert lib.dvae_mel_to_frames(p, p, w, *dims, 0, s) == E_ and lib.dvae_frames_to_mel(p, w, *dims, s) == E_
        assert lib.dvae_permute_102(p, w, dims[0], dims[1], 4 * dims[2], s) == E_
        assert lib.dvae_mel_to_chunks(p, w, dims[0], 4, dims[1], dims[2], s) == E_
        assert lib.dvae_chunks_to_mel(p, w, *dims, 0.0, 1.0, 1, s) == E_
    assert lib.dvae_permute_102(p, w, 1, 1, 6, s) == E_ and lib.dvae_permute_102(p, w, 1, 1, 2, s) == E_
    assert lib.dvae_mel_to_chunks(p, w, 1, -1, 1, 1, s) == E_
    for dims in ((0, 1), (1, 0)):
        assert lib.dvae_transpose(p, w, *dims, s) == E_ and lib.dvae_conv_pack_w(p, w, *dims, s) == E_
        assert lib.dvae_conv_pack_wt(p, w, *dims, s) == E_ and lib.dvae_conv_unpack_add_w(p, w, *dims, s) == E_
    assert lib.dvae_transpose(None, w, 1, 1, s) == E_ and lib.dvae_conv_unpack_add_w(p, None, 1, 1, s) == E_
    for dims in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        assert lib.dvae_gather_crop(p, i32.ptr, i32.ptr, i32.ptr, w, *dims, s) == E_
        assert lib.dvae_conversion_latents(p, p, p, w, w, *dims, s) == E_
    assert lib.dvae_gather_crop(p, None, i32.ptr, i32.ptr, w, 1, 1, 1, 1, s) == E_
    assert lib.dvae_conversion_latents(p, p, None, w, w, 1, 1, 1, 1, s) == E_
    assert lib.dvae_mul_div(p, p, None, w, 4, s) == E_ and lib.dvae_mul_div(p, p, p, w, 0, s) == E_
    guards(x, y, o, ws, i32)
    assert np.array_equal(o.bits(), before) and not ws.bits().any()
    # ... and a good call is taken
    ok(lib.dvae_mul_div(p, p, q, w, 64, s))
    assert (o.np() == 1.0).all()
