"""dvae_loss_fwd_sched / dvae_loss_bwd_sched of csrc/elem.hip on the MI355X through the C ABI: bit for bit dvae_loss_fwd /
dvae_loss_bwd while no free bits are given (the weights read from the device), and with free bits against the float64
restatement of tests/kl_sched_ref.py, within the bounds derived there; the gate and the free counts exactly, because the
inputs keep every column ten bounds away from its lambda (tests/test_kl_sched_ref.py proves that for every shape here).
Every buffer a launch may write is a guarded one of tests/kernel_harness.py."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import assert_same_bits, Buf, EINVAL, F32, F64, guards, L, ok, P, st, Worst
import dvae_amd  # noqa: E402,F401
from dvae_amd import _lib  # noqa: E402
import elem_ref as E  # noqa: E402
import kl_sched_ref as R  # noqa: E402

WORST = Worst("test_hip_kl_sched.py", sort=True, ratio_fn=E.worst_ratio)
note = WORST.note


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    WORST.report()


def bufs(d):
    return {k: Buf(None, data=d[k]) for k in E.LOSS_KEYS}


def loss_desc(b, d, weights=None):
    desc = _lib.LossDesc()
    for k in E.LOSS_KEYS:
        setattr(desc, k, b[k] if isinstance(b[k], int) else b[k].ptr)
    desc.n, desc.nq, desc.ns = d["n"], d["nq"], d["ns"]
    for k in E.SCALE_KEYS[:3]:
        setattr(desc, k, float(d[k]))
    # the scheduled calls must ignore the descriptor's weights: they get NaN there
    desc.mse_cof, desc.kl_cof = (float("nan"), float("nan")) if weights is None else (float(weights[0]), float(weights[1]))
    return desc


def coef_buf(c0, c1):
    return Buf(None, data=np.asarray([c0, c1, 0, 0, 0, 0, 0, 0], F32))


def sched_of(coef, lam, D):
    s = _lib.LossSched()
    s.coef, s.free_bits, s.D = coef.ptr, P(lam), D
    return s


def fwd_legacy(b, d, weights):
    out, ws = Buf((8,)), Buf((L().dvae_loss_ws_bytes(1),), torch.uint8)
    ok(L().dvae_loss_fwd(ctypes.byref(loss_desc(b, d, weights)), out.ptr, ws.ptr, st()))
    guards(out, ws)
    return out


def grad_bufs(d, null=()):
    n, nq, ns = d["n"], d["nq"], d["ns"]
    return [None if k in null else Buf((m,)) for k, m in zip(range(10), (n, n, n, n, nq, nq, nq, nq, ns, ns))]


def bwd_legacy(b, d, weights, g8, null=()):
    outs = grad_bufs(d, null)
    ok(L().dvae_loss_bwd(ctypes.byref(loss_desc(b, d, weights)), g8.ptr, *[P(o) for o in outs], st()))
    guards(*outs)
    return outs


def fwd_sched(b, d, coef, lam, D):
    out, aux, ws = Buf((8,)), Buf((4 + 4 * D,)), Buf((L().dvae_loss_ws_bytes(1),), torch.uint8)
    s = sched_of(coef, lam, D)
    ok(L().dvae_loss_fwd_sched(ctypes.byref(loss_desc(b, d)), ctypes.byref(s), out.ptr, aux.ptr, ws.ptr, st()))
    guards(out, aux, ws, coef, lam)
    return out, aux


def bwd_sched(b, d, coef, lam, D, aux, g8, null=()):
    outs = grad_bufs(d, null)
    s = sched_of(coef, lam, D)
    before = aux.bits()
    ok(L().dvae_loss_bwd_sched(ctypes.byref(loss_desc(b, d)), ctypes.byref(s), aux.ptr, g8.ptr, *[P(o) for o in outs], st()))
    guards(*outs, aux, coef, lam)
    assert np.array_equal(aux.bits(), before), "backward wrote into aux"
    return outs


# ------------------------------------------------------------------ without free bits: the legacy bits
@pytest.mark.parametrize("n,nq,ns", R.bit_cases(), ids=lambda v: str(v))
def test_without_free_bits_the_bits_are_the_legacy_calls(n, nq, ns):
    d = E.loss_inputs(n, nq, ns, "R", n % 1000 + nq)
    b = bufs(d)
    w = (F32(10.0), F32(3.0)) if n % 2 else (F32(0.37), F32(7.25))
    coef = coef_buf(*w)
    legacy = fwd_legacy(b, d, w)
    for D in R.divisors(nq):
        out, aux = fwd_sched(b, d, coef, None, D)
        what = f"n={n} nq={nq} ns={ns} D={D}"
        assert_same_bits(out, legacy.np(), what + " out8")
        a = aux.np()
        assert_same_bits(a[:2], legacy.np()[5:7], what + " aux[0..1]")
        assert (a[2:4] == 0).all() and (a[4 + 2 * D:] == 1).all(), what
        for gname, g8v in E.G8.items():
            if n > 4099 and (gname != "random" or D != R.divisors(nq)[-1]):
                continue
            g8 = Buf(None, data=g8v)
            ref = bwd_legacy(b, d, w, g8)
            got = bwd_sched(b, d, coef, None, D, aux, g8)
            for k in range(10):
                assert_same_bits(got[k], ref[k].np(), f"{what} {gname} gradient {k}")


def test_the_weights_come_from_the_device():
    n, nq, ns, D = 1023, 255, 300, 5
    d = E.loss_inputs(n, nq, ns, "R", 3)
    b, g8 = bufs(d), Buf(None, data=E.G8["random"])
    coef = coef_buf(10.0, 3.0)
    seen = []
    for w in ((F32(10.0), F32(3.0)), (F32(2.5), F32(0.0)), (F32(0.0), F32(1e-3))):
        coef.t.copy_(torch.tensor([w[0], w[1], 0, 0, 0, 0, 0, 0], dtype=torch.float32))      # the same descriptor and buffers
        out, aux = fwd_sched(b, d, coef, None, D)
        assert_same_bits(out, fwd_legacy(b, d, w).np(), f"weights {w}")
        got, ref = bwd_sched(b, d, coef, None, D, aux, g8), bwd_legacy(b, d, w, g8)
        for k in range(10):
            assert_same_bits(got[k], ref[k].np(), f"weights {w} gradient {k}")
        seen.append(out.bits()[0])
    assert len(set(seen)) == 3


# ------------------------------------------------------------------ free bits against the float64 restatement
def _cases():
    return [(rows, D, single) for rows, D in R.SHAPES for single in (("free", "on") if D == 1 else ("free",))]


@pytest.mark.parametrize("rows,D,single", _cases())
def test_free_bits_against_the_restatement(rows, D, single):
    coefv = (F32(10.0), F32(3.0))
    for n in R.NS:
        d = R.inputs(rows, D, n, 1000 + rows + D)
        lamv = R.free_bits_for(d, single)
        b, coef, lam = bufs(d), coef_buf(*coefv), Buf(None, data=lamv)
        out, aux = fwd_sched(b, d, coef, lam, D)
        o, a = out.np(), aux.np()
        what = f"rows={rows} D={D} n={n} {single}"
        ref8, refa, tol8, tola = R.fwd_bounds(d, coefv, lamv, o, a)
        assert_same_bits(o[1:], fwd_legacy(b, d, coefv).np()[1:], what + ": out8[1..7] are the raw terms")
        note("kl_dim", a[4:4 + 2 * D], refa[4:4 + 2 * D], tola[4:4 + 2 * D], what)
        note("aux clamped", a[:2], refa[:2], tola[:2], what)
        note("out8[0]", o[0], ref8[0], tol8[0], what)
        assert np.array_equal(a[4 + 2 * D:].astype(F64), refa[4 + 2 * D:]), what + ": the gate"
        assert np.array_equal(a[2:4].astype(F64), refa[2:4]), what + ": the free counts"
        gate = refa[4 + 2 * D:].reshape(2, D)
        free = [np.tile(gate[k] == 0, rows) for k in range(2)]
        for gname, g8v in E.G8.items():
            outs = bwd_sched(b, d, coef, lam, D, aux, Buf(None, data=g8v))
            refs, tols = R.bwd_bounds(d, coefv, g8v, gate)
            legacy = bwd_legacy(b, d, coefv, Buf(None, data=g8v))
            for k in (0, 1, 2, 3, 8, 9):        # reconstructions and style: untouched by free bits
                assert_same_bits(outs[k], legacy[k].np(), f"{what} {gname} gradient {k}")
            for k in range(4, 8):
                got = outs[k].np()
                note("d" + ("mu" if k % 2 == 0 else "lv"), got, refs[k], tols[k], f"{what} {gname} {E.LOSS_KEYS[2 + k]}")
                f = free[(k - 4) // 2]
                assert_same_bits(got[~f], legacy[k].np()[~f], f"{what} {gname} gradient {k}: a penalised dimension")
                if gname == "total":            # nothing but g8[0] arrives: a free dimension gets exactly zero
                    assert (got[f] == 0).all(), f"{what}: a free dimension took a gradient from the total"


@pytest.mark.parametrize("rows,D", [(3, 5), (4, 32), (300, 257)])
def test_every_dimension_free_and_every_dimension_penalised(rows, D):
    n, coefv = 4, (F32(10.0), F32(3.0))
    d = R.positive_inputs(rows, D, n, 2000 + rows + D)
    b, coef = bufs(d), coef_buf(*coefv)
    g8 = Buf(None, data=E.G8["total"])
    # lambda = +large: all free, the latent gradients are zero and LOSS carries the sum of the lambdas
    big = np.full(D, 1e6, F32)
    R.check_margin(d, big)
    out, aux = fwd_sched(b, d, coef, Buf(None, data=big), D)
    o, a = out.np(), aux.np()
    assert (a[2:4] == D).all() and (a[4 + 2 * D:] == 0).all()
    assert_same_bits(a[:2], F32([big.astype(F64).sum()] * 2), "sum of the lambdas")
    ref8, _, tol8, _ = R.fwd_bounds(d, coefv, big, o, a)
    note("out8[0] all free", o[0], ref8[0], tol8[0], f"rows={rows} D={D}")
    outs = bwd_sched(b, d, coef, Buf(None, data=big), D, aux, g8)
    for k in range(4, 8):
        assert (outs[k].np() == 0).all()
    # lambda = 0 below a strictly positive KL: all penalised, the bits of the call without free bits
    zero = Buf(None, data=np.zeros(D, F32))
    R.check_margin(d, np.zeros(D, F32))
    out0, aux0 = fwd_sched(b, d, coef, zero, D)
    outn, auxn = fwd_sched(b, d, coef, None, D)
    assert (aux0.np()[2:4] == 0).all() and (aux0.np()[4 + 2 * D:] == 1).all()
    assert_same_bits(aux0.np()[4:], auxn.np()[4:], "kl_dim and gate")
    assert_same_bits(out0.np()[1:], outn.np()[1:], "raw terms")
    for gname, g8v in E.G8.items():
        gb = Buf(None, data=g8v)
        a_, b_ = bwd_sched(b, d, coef, zero, D, aux0, gb), bwd_sched(b, d, coef, None, D, auxn, gb)
        for k in range(10):
            assert_same_bits(a_[k], b_[k].np(), f"lambda = 0, {gname}, gradient {k}")


def test_null_outputs_and_offsets_into_one_tensor():
    rows, D, n, ns = 4, 32, 1023, 16
    d = R.inputs(rows, D, n, 11, ns=ns)
    nq = rows * D
    lamv = R.free_bits_for(d)
    b, coef, lam, g8 = bufs(d), coef_buf(10.0, 3.0), Buf(None, data=lamv), Buf(None, data=E.G8["random"])
    out, aux = fwd_sched(b, d, coef, lam, D)
    full = bwd_sched(b, d, coef, lam, D, aux, g8)
    for null in ((0,), (3,), (4, 5), (6, 7), (8, 9), (0, 1, 2, 3), (4, 5, 6, 7, 8, 9)):
        outs = bwd_sched(b, d, coef, lam, D, aux, g8, null)
        for k in range(10):
            assert (outs[k] is None) == (k in null)
            assert outs[k] is None or np.array_equal(outs[k].bits(), full[k].bits()), f"null {null}: output {k} changed"
    # what ops.LossGVAE2SchedFn passes: the halves as offsets into one buffer, the gradients too (n = 1023: 4 n is not a
    # multiple of 16, so the second half is pushed to the next 16-byte boundary the way a [2 Bh, 80, T] tensor's is)
    n4 = 1024
    cat = lambda p, q, m: Buf(None, data=np.concatenate([d[p], np.zeros(m - d[p].size, F32), d[q]]))
    rec, hat = cat("recon1", "recon2", n4), cat("recon1_hat", "recon2_hat", n4)
    qmu, qlv = cat("q1_mu", "q2_mu", nq), cat("q1_lv", "q2_lv", nq)
    pb = dict(b, recon1=rec.ptr, recon2=rec.ptr + 4 * n4, recon1_hat=hat.ptr, recon2_hat=hat.ptr + 4 * n4, q1_mu=qmu.ptr,
              q2_mu=qmu.ptr + 4 * nq, q1_lv=qlv.ptr, q2_lv=qlv.ptr + 4 * nq)
    out2, aux2 = fwd_sched(pb, d, coef, lam, D)
    assert np.array_equal(out2.bits(), out.bits()) and np.array_equal(aux2.bits(), aux.bits())
    grec, ghat, gmu, glv, gsm, gsl = Buf((n4 + n,)), Buf((n4 + n,)), Buf((2 * nq,)), Buf((2 * nq,)), Buf((ns,)), Buf((ns,))
    s = sched_of(coef, lam, D)
    ok(L().dvae_loss_bwd_sched(ctypes.byref(loss_desc(pb, d)), ctypes.byref(s), aux2.ptr, g8.ptr, grec.ptr, grec.ptr + 4 * n4,
                               ghat.ptr, ghat.ptr + 4 * n4, gmu.ptr, glv.ptr, gmu.ptr + 4 * nq, glv.ptr + 4 * nq, gsm.ptr,
                               gsl.ptr, st()))
    guards(grec, ghat, gmu, glv, gsm, gsl)
    for got, k1, k2 in ((grec, 0, 1), (ghat, 2, 3)):
        assert np.array_equal(got.bits()[:n], full[k1].bits()) and np.array_equal(got.bits()[n4:], full[k2].bits())
    for got, k1, k2 in ((gmu, 4, 6), (glv, 5, 7)):
        assert np.array_equal(got.bits(), np.concatenate([full[k1].bits(), full[k2].bits()]))
    assert np.array_equal(gsm.bits(), full[8].bits()) and np.array_equal(gsl.bits(), full[9].bits())


def test_two_runs_give_the_same_bits():
    for rows, D in ((300, 257), (2, 1024), (64, 64)):
        d = R.inputs(rows, D, 1023, 5)
        b, coef, lam = bufs(d), coef_buf(10.0, 3.0), Buf(None, data=R.free_bits_for(d))
        o1, a1 = fwd_sched(b, d, coef, lam, D)
        o2, a2 = fwd_sched(b, d, coef, lam, D)
        assert np.array_equal(a1.bits(), a2.bits()) and np.array_equal(o1.bits(), o2.bits())


def test_einval_writes_nothing():
    rows, D, n = 4, 32, 8
    d = R.inputs(rows, D, n, 1)
    b, coef, lam, g8 = bufs(d), coef_buf(10.0, 3.0), Buf(None, data=np.zeros(D, F32)), Buf(None, data=E.G8["ones"])
    out, aux, ws = Buf((8,)), Buf((4 + 4 * D,)), Buf((L().dvae_loss_ws_bytes(1),), torch.uint8)
    auxr = Buf(None, data=np.ones(4 + 4 * D, F32))
    grads = grad_bufs(d)
    lib, s_ = L(), st()
    desc = loss_desc(b, d)

    def both(sched, aux_f, aux_b, dsc=desc):
        sp = None if sched is None else ctypes.byref(sched)
        assert lib.dvae_loss_fwd_sched(ctypes.byref(dsc), sp, out.ptr, aux_f, ws.ptr, s_) == EINVAL
        assert lib.dvae_loss_bwd_sched(ctypes.byref(dsc), sp, aux_b, g8.ptr, *[g.ptr for g in grads], s_) == EINVAL

    def sched(coef_p=coef.ptr, lam_p=lam.ptr, D_=D):
        s = _lib.LossSched()
        s.coef, s.free_bits, s.D = coef_p, lam_p, D_
        return s

    both(None, aux.ptr, auxr.ptr)                                   # no schedule
    both(sched(coef_p=None), aux.ptr, auxr.ptr)                     # a null coef
    both(sched(), None, None)                                       # a null aux
    for bad_D in (0, -1, _lib.LOSS_MAX_D + 1, 5, 3):                # out of range; not dividing nq = 128
        both(sched(D_=bad_D), aux.ptr, auxr.ptr)
    both(sched(coef_p=coef.ptr + 2), aux.ptr, auxr.ptr)             # misaligned coef, free_bits, aux
    both(sched(lam_p=lam.ptr + 1), aux.ptr, auxr.ptr)
    both(sched(), aux.ptr + 2, auxr.ptr + 2)
    bad = loss_desc(dict(b, recon1=b["recon1"].ptr + 4), d)         # ... and what the legacy calls refuse
    both(sched(), aux.ptr, auxr.ptr, bad)
    both(sched(), aux.ptr, auxr.ptr, loss_desc(b, dict(d, nq=0)))
    good = sched()
    assert lib.dvae_loss_fwd_sched(ctypes.byref(desc), ctypes.byref(good), None, aux.ptr, ws.ptr, s_) == EINVAL
    assert lib.dvae_loss_fwd_sched(ctypes.byref(desc), ctypes.byref(good), out.ptr, aux.ptr, None, s_) == EINVAL
    assert lib.dvae_loss_bwd_sched(ctypes.byref(desc), ctypes.byref(good), auxr.ptr, None, *[g.ptr for g in grads], s_) == EINVAL
    ptrs = [g.ptr for g in grads]
    assert lib.dvae_loss_bwd_sched(ctypes.byref(desc), ctypes.byref(good), auxr.ptr, g8.ptr, *ptrs[:5], None, *ptrs[6:], s_) == EINVAL
    assert lib.dvae_loss_bwd_sched(ctypes.byref(desc), ctypes.byref(good), auxr.ptr, g8.ptr, ptrs[0] + 4, *ptrs[1:], s_) == EINVAL
    guards(out, aux, ws, auxr, *grads)
    for buf in (out, aux, *grads):
        assert buf.poisoned().all(), "a refused call wrote an output"
    assert ws.poisoned().all()
    # D = nq (one row) and D = DVAE_LOSS_MAX_D are inside the range
    d1 = R.inputs(1, _lib.LOSS_MAX_D, 4, 2)
    o, a = fwd_sched(bufs(d1), d1, coef, None, _lib.LOSS_MAX_D)
    assert np.isfinite(o.np()).all() and np.isfinite(a.np()).all()
