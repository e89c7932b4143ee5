"""The factor-penalty kernels of csrc/factor.hip (dvae_factor_fwd, dvae_factor_bwd) on the MI355X
through the C ABI, against the float64 restatement of tests/factor_ref.py.

Every statistic, every L and every element of dz, dq_mu and dq_lv is held to the bound derived in factor_ref (from 2^-24 and
the operation counts on the fp32 inputs, never from what the kernel gives); what the contract calls bit-exact is compared bit
for bit: two launches, a row among other rows, the gradients under zero weights.  Every buffer a launch may write is a guarded
one of tests/kernel_harness.py, pre-filled with 0xFF.  Each shape runs twice: with a row planted far from every column (its
softmax is decided by roundings: its L is held, its gradients are finite, the bounds it enters say little) and without (the
bounds are tight).  The worst error / bound per shape is printed at the module's end.

Worst error / bound on the MI355X, per (Bh, S, Cn), without / with the far row: L 0.122 / 0.215 (1, 1, 1), 0.134 / 0.228
(1, 2, 2), 0.200 / 0.200 (3, 2, 4), 0.160 / 0.160 (32, 4, 28), 0.168 / 0.168 (33, 4, 28), 0.164 / 0.164 (65, 16, 48), 0.123 at
N = 1024; own_i at most 0.165; the statistics at most 0.034 / 0.086; without the far row dz at most 0.085, dq_mu 0.052, dq_lv
0.038.  With the far row dz reaches 0.998 and dq_mu, dq_lv 1.000 from (3, 2, 4) on: the far row's softmax winner is decided
by roundings, fp32 and float64 pick different columns, the error of that p IS 1 and the bound allows 1 (times a factor of the
order of 1e8 that swamps every other term of those elements); the elements it does not enter stay where the other variant has
them.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
from kernel_harness import Buf, EINVAL, F32, F64, guards, L, ok, Pad, st, Worst
import dvae_amd  # noqa: E402,F401
import factor_ref as R  # noqa: E402

WORST = Worst("test_hip_factor.py (rows: Bh, S, Cn and whether a far row is planted)")
note = WORST.note


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    WORST.report()


class Launch:
    """one forward and one backward of a case through the C ABI, everything written into guarded buffers"""

    def __init__(self, z, mu, lv, S, weights, gscale=None, bwd=True, pen=True):
        N, D = z.shape
        self.N, self.D, self.S = N, D, S
        self.z, self.mu, self.lv = Pad(z), Pad(mu), Pad(lv)
        self.w = Pad(np.asarray(weights, F32))
        self.gs = None if gscale is None else Pad(np.asarray([gscale], F32))
        nws = L().dvae_factor_ws_bytes(N)
        assert nws == 4 * N
        self.L, self.stats, self.ws, self.pen = Buf((N, D + 3)), Buf((5,)), Buf((nws // 4,)), Buf((1,))
        ok(L().dvae_factor_fwd(self.z.ptr, self.mu.ptr, self.lv.ptr, N, D, S, self.w.ptr, self.L.ptr, self.stats.ptr,
                               self.pen.ptr if pen else None, self.ws.ptr, st()), "dvae_factor_fwd")
        assert self.pen.poisoned().all() if not pen else np.array_equal(self.pen.bits(), self.stats.bits()[4:])
        self.dz = self.dmu = self.dlv = None
        if bwd:
            self.dz, self.dmu, self.dlv = Buf((N, D)), Buf((N, D)), Buf((N, D))
            ok(L().dvae_factor_bwd(self.z.ptr, self.mu.ptr, self.lv.ptr, self.L.ptr, N, D, S, self.w.ptr,
                                   None if self.gs is None else self.gs.ptr, self.dz.ptr, self.dmu.ptr, self.dlv.ptr, st()),
               "dvae_factor_bwd")
        guards(self.L, self.stats, self.ws, self.pen, self.dz, self.dmu, self.dlv, self.z.buf, self.mu.buf, self.lv.buf, self.w.buf)

    def outputs(self):
        return [b for b in (self.L, self.stats, self.ws, self.dz, self.dmu, self.dlv) if b is not None]


_REF = {}


def reference(Bh, S, Cn, far):
    """the float64 side of a case, computed once and shared"""
    key = (Bh, S, Cn, far)
    if key not in _REF:
        c = R.kernel_case(Bh, S, Cn, far=far)
        f = R.forward(c["z"], c["mu"], c["lv"], S, *R.WEIGHTS)
        tau = R.tau_table(c["z"], c["mu"], c["lv"], S, f["t"])
        _REF[key] = dict(c, f=f, tau=tau, BL=R.L_bound(f["t"], tau, f["L"]))
    return _REF[key]


@pytest.mark.parametrize("far", [True, False], ids=["far", "near"])
@pytest.mark.parametrize("Bh,S,Cn", R.SHAPES)
def test_against_float64(Bh, S, Cn, far):
    c = reference(Bh, S, Cn, far)
    f, tau, BL = c["f"], c["tau"], c["BL"]
    N, D = 2 * Bh, S + Cn
    key = f"{Bh},{S},{Cn} {'far' if far else 'near'}"
    a = Launch(c["z"], c["mu"], c["lv"], S, R.WEIGHTS)
    got_L = a.L.np()
    assert np.all(np.isfinite(got_L)), "a row far from every column must keep a finite L"
    assert not a.L.poisoned().any() and not a.stats.poisoned().any() and not a.ws.poisoned().any()
    if far:
        assert f["L"][0, D + 2] < -1e3 * D                                   # the far row is far
    if c["hot"] is not None:
        gam = np.exp(f["t"][c["hot"], :, D + 2] - f["L"][c["hot"], D + 2])
        assert gam[c["hot"]] > 1 - 1e-12                                     # the one-hot row is one-hot
    note((key, "L"), got_L, f["L"], BL, f"far={far}")
    own_tau = tau[np.arange(N), np.arange(N), D + 2]
    note((key, "own"), a.ws.np(), f["own"], own_tau + R.FLOOR, f"far={far}")
    sb = R.stats_bound(BL, own_tau, f["stats"], S, *R.WEIGHTS)
    note((key, "stats"), a.stats.np(), f["stats"], sb, f"far={far}")
    # the gradients, against the closed forms in float64 with their own L; the kernel read the L it wrote
    gz, gm, gl = R.gradients(c["z"], c["mu"], c["lv"], S, *R.WEIGHTS)
    bz, bm, bl = R.gradient_bounds(c["z"], c["mu"], c["lv"], S, *R.WEIGHTS, f["t"], tau, f["L"], BL)
    for name, buf, ref, bound in (("dz", a.dz, gz, bz), ("dmu", a.dmu, gm, bm), ("dlv", a.dlv, gl, bl)):
        got = buf.np()
        assert np.all(np.isfinite(got)), f"{name}: the gradients of a far row, and those it enters, must stay finite"
        note((key, name), got, ref, bound, f"far={far}")
    # a second launch gives the same bits
    b = Launch(c["z"], c["mu"], c["lv"], S, R.WEIGHTS)
    for x, y in zip(a.outputs(), b.outputs()):
        assert np.array_equal(x.bits(), y.bits()), "a second launch gives the same bits"


@pytest.mark.parametrize("Bh,S,Cn", [(3, 2, 4), (33, 4, 28)])
def test_a_row_does_not_depend_on_the_other_rows(Bh, S, Cn):
    """z is an argument of its own: with the columns (mu, lv) kept, a row's L depends on that row of z alone"""
    c = reference(Bh, S, Cn, True)
    N = 2 * Bh
    a = Launch(c["z"], c["mu"], c["lv"], S, R.WEIGHTS, bwd=False).L.bits()
    rs = np.random.RandomState(5)
    for keep in (0, 1, N - 1):
        z = (c["z"] + rs.randn(*c["z"].shape)).astype(F32)
        z[keep] = c["z"][keep]
        b = Launch(z, c["mu"], c["lv"], S, R.WEIGHTS, bwd=False).L.bits()
        assert np.array_equal(a[keep], b[keep]), f"row {keep}: among other rows"
        assert not np.array_equal(a, b)


def test_gscale_scales_the_gradients():
    """the incoming gradient of the penalty multiplies the three coefficients: 2 is exact"""
    c = reference(3, 2, 4, False)
    one = Launch(c["z"], c["mu"], c["lv"], 2, R.WEIGHTS, gscale=1.0)
    none = Launch(c["z"], c["mu"], c["lv"], 2, R.WEIGHTS, pen=False)      # and without the penalty's second home
    two = Launch(c["z"], c["mu"], c["lv"], 2, R.WEIGHTS, gscale=2.0)
    for x, y, t in zip((one.dz, one.dmu, one.dlv), (none.dz, none.dmu, none.dlv), (two.dz, two.dmu, two.dlv)):
        assert np.array_equal(x.bits(), y.bits())
        assert np.array_equal((2.0 * x.np()).view(np.uint32), t.np().view(np.uint32))


@pytest.mark.parametrize("Bh,S,Cn", [(3, 2, 4), (65, 16, 48)])
def test_zero_weights_write_positive_zero(Bh, S, Cn):
    c = reference(Bh, S, Cn, True)
    z = c["z"].copy()
    z[1, 0] = np.nan
    a = Launch(z, c["mu"], c["lv"], S, (0.0, 0.0), gscale=np.nan)
    for buf in (a.dz, a.dmu, a.dlv):
        assert (buf.bits() == 0).all(), "zero weights: every gradient element is +0.0"
    assert np.isnan(a.stats.np()).any()                  # the NaN is in the statistics, and stays there
    # one weight alone is not zero weights
    b = Launch(c["z"], c["mu"], c["lv"], S, (0.0, 0.5))
    assert np.abs(b.dz.np()).max() > 0


def test_refusals_leave_the_outputs_untouched():
    c = reference(3, 2, 4, False)
    z, mu, lv, w = Pad(c["z"]), Pad(c["mu"]), Pad(c["lv"]), Pad(np.asarray(R.WEIGHTS, F32))
    N, D, S = 6, 6, 2
    big = Pad(np.zeros((2, 65), F32))
    many = Pad(np.zeros((R.MAX_N + 1, 2), F32))

    def fwd(**kw):
        a = dict(z=z.ptr, mu=mu.ptr, lv=lv.ptr, N=N, D=D, S=S, w=w.ptr)
        outs = dict(L=Buf((max(N, kw.get("N", N)), 70)), stats=Buf((5,)), ws=Buf((R.MAX_N + 1,)), pen=Buf((1,)))
        ptrs = {k: v.ptr for k, v in outs.items()}
        a.update(ptrs)
        a.update(kw)
        rc = L().dvae_factor_fwd(a["z"], a["mu"], a["lv"], a["N"], a["D"], a["S"], a["w"], a["L"], a["stats"], a["pen"], a["ws"],
                                 st())
        assert rc == EINVAL, (kw, rc)
        guards(*outs.values())
        assert all(b.poisoned().all() for b in outs.values()), f"{kw}: a refused call wrote an output"

    def bwd(**kw):
        Lb = Pad(np.zeros((R.MAX_N + 1, 70), F32))
        a = dict(z=z.ptr, mu=mu.ptr, lv=lv.ptr, L=Lb.ptr, N=N, D=D, S=S, w=w.ptr, gs=None)
        outs = dict(dz=Buf((R.MAX_N + 1, 65)), dmu=Buf((R.MAX_N + 1, 65)), dlv=Buf((R.MAX_N + 1, 65)))
        a.update({k: v.ptr for k, v in outs.items()})
        a.update(kw)
        rc = L().dvae_factor_bwd(a["z"], a["mu"], a["lv"], a["L"], a["N"], a["D"], a["S"], a["w"], a["gs"], a["dz"], a["dmu"],
                                 a["dlv"], st())
        assert rc == EINVAL, (kw, rc)
        guards(*outs.values())
        assert all(b.poisoned().all() for b in outs.values()), f"{kw}: a refused call wrote an output"

    shapes = (dict(N=0), dict(N=-2), dict(S=0), dict(S=D), dict(S=D + 1), dict(D=0), dict(D=1, S=1),
              dict(D=65, S=2, N=2, z=big.ptr, mu=big.ptr, lv=big.ptr),
              dict(N=R.MAX_N + 1, D=2, S=1, z=many.ptr, mu=many.ptr, lv=many.ptr))
    for kw in (dict(z=None), dict(mu=None), dict(lv=None), dict(w=None), dict(L=None), dict(stats=None), dict(ws=None)) + shapes:
        fwd(**kw)
    for kw in (dict(z=None), dict(mu=None), dict(lv=None), dict(w=None), dict(L=None), dict(dz=None), dict(dmu=None),
               dict(dlv=None)) + shapes:
        bwd(**kw)
    assert L().dvae_factor_ws_bytes(0) == -1 and L().dvae_factor_ws_bytes(R.MAX_N + 1) == -1
    assert L().dvae_factor_ws_bytes(R.MAX_N) == 4 * R.MAX_N


def test_the_largest_launch():
    """N = DVAE_FACTOR_MAX_N rows at D = 64: the LDS rows are full; finite, in bounds (the guards), the same bits twice, and
    the statistics of independent factorised posteriors at their known scale"""
    rs = np.random.RandomState(3)
    N, S, D = R.MAX_N, 16, 64
    mu, lv = rs.randn(N, D).astype(F32), rs.uniform(-2.0, 0.0, (N, D)).astype(F32)
    z = (mu + np.exp(0.5 * lv) * rs.randn(N, D)).astype(F32)
    a = Launch(z, mu, lv, S, R.WEIGHTS)
    b = Launch(z, mu, lv, S, R.WEIGHTS)
    for x, y in zip(a.outputs(), b.outputs()):
        assert np.isfinite(x.np()).all() and np.array_equal(x.bits(), y.bits())
    rows = np.array([0, 1, 511, 1023])                  # float64 for four rows against all the columns
    t = R.sets(R.table(z[rows], mu, lv), S)
    L64 = R.lse(t)
    note((f"{N // 2},{S},{D - S} largest", "L"), a.L.np()[rows], L64, R.L_bound(t, R.tau_table(z[rows], mu, lv, S, t), L64),
         "the largest launch")
