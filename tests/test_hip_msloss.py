"""The smoothing-penalty kernels of csrc/msloss.hip (dvae_msloss_fwd, dvae_msloss_bwd) on the MI355X
through the C ABI, against the float64 restatement of tests/msloss_ref.py.

The penalty, every statistic and every element of dy is held to the bound derived in msloss_ref (from 2^-53, 2^-24 and the
operation counts, never from what the kernel gives) with NO element left out: the stabiliser makes every element well
conditioned.  What the contract calls bit-exact is compared bit for bit: two launches, a row among other rows, gscale = 2, the
gradient under zero weights.  Every buffer a launch may write is a guarded one of tests/kernel_harness.py, pre-filled with
0xFF.  The worst error / bound per shape and output is printed at the module's end.

Worst error / bound on the MI355X over the five shapes: L_ms 0.501, L_gv 0.532, msd_db 0.722, gv_ratio_db 0.408, penalty 0.729,
dy 0.997 (0.695 at (1, 1, 8, 8)): the float64 parts of the bounds are of the order of 1e-14 relative, so what is seen is the one
rounding to fp32 at the store, half a spacing at the most, over up to 40 960 elements.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import Buf, EINVAL, F32, F64, guards, L, ok, Pad, st, Worst
import dvae_amd  # noqa: E402,F401
import msloss_ref as R  # noqa: E402

WORST = Worst("test_hip_msloss.py (rows: Bh, C, T, D)")
note = WORST.note


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    WORST.report()


def ws_doubles(N, C):
    return 3 * N * -(-C // R.BINS) + 2 * N * C


class Launch:
    """one forward and one backward of a case through the C ABI, everything written into guarded buffers"""

    def __init__(self, y, x1, x2, D, weights=R.WEIGHTS, floor=R.FLOOR, gscale=None, bwd=True, pen=True):
        N, C, T = y.shape
        self.y, self.x1, self.x2 = Pad(y), Pad(x1), Pad(x2)
        self.w = Pad(np.asarray(weights, F32))
        self.tw = Buf(data=R.twiddle(D))
        self.gs = None if gscale is None else Pad(np.asarray([gscale], F32))
        nws = L().dvae_msloss_ws_bytes(N, C)
        assert nws == 8 * ws_doubles(N, C)
        self.stats, self.ws, self.pen = Buf((5,)), Buf((nws // 8,), dtype=torch.float64), Buf((1,))
        ok(L().dvae_msloss_fwd(self.y.ptr, self.x1.ptr, self.x2.ptr, N // 2, C, T, D, floor, self.tw.ptr, self.w.ptr,
                               self.stats.ptr, self.pen.ptr if pen else None, self.ws.ptr, st()), "dvae_msloss_fwd")
        assert self.pen.poisoned().all() if not pen else np.array_equal(self.pen.bits(), self.stats.bits()[4:])
        self.dy = None
        if bwd:
            self.dy = Buf((N, C, T))
            ok(L().dvae_msloss_bwd(self.y.ptr, self.x1.ptr, self.x2.ptr, N // 2, C, T, D, floor, self.tw.ptr, self.w.ptr,
                                   None if self.gs is None else self.gs.ptr, self.ws.ptr, self.dy.ptr, st()), "dvae_msloss_bwd")
        guards(self.stats, self.ws, self.pen, self.dy, self.y.buf, self.x1.buf, self.x2.buf, self.w.buf, self.tw)

    def outputs(self):
        return [b for b in (self.stats, self.ws, self.dy) if b is not None]


_REF = {}


def reference(Bh, C, T, D):
    """the float64 side of a case, computed once and shared"""
    key = (Bh, C, T, D)
    if key not in _REF:
        c = R.kernel_case(Bh, C, T, D)
        r = R.evaluate(c["y"], c["x1"], c["x2"], D)
        _REF[key] = dict(c, r=r, bounds=R.bounds(r))
    return _REF[key]


@pytest.mark.parametrize("Bh,C,T,D", R.SHAPES)
def test_against_float64(Bh, C, T, D):
    c = reference(Bh, C, T, D)
    r, (sb, db) = c["r"], c["bounds"]
    key = f"{Bh},{C},{T},{D}"
    a = Launch(c["y"], c["x1"], c["x2"], D)
    assert not a.stats.poisoned().any() and not a.ws.poisoned().any() and not a.dy.poisoned().any()
    got = a.stats.np()
    for k, name in enumerate(("L_ms", "L_gv", "msd_db", "gv_ratio_db", "penalty")):
        note((key, name), got[k], r["stats"][k], sb[k], key)
    note((key, "dy"), a.dy.np(), r["dy"], db, key)                           # every element: none is left out
    assert (a.dy.bits()[0, C - 1] == 0).all(), "a constant trajectory: a gradient of exactly +0.0"
    # what the forward pass leaves for the backward one: m and 2 (g - g^x) / (v + eps_gv) per (row, bin)
    N = 2 * Bh
    tail = a.ws.np()[3 * N * -(-C // R.BINS):].reshape(2, N, C)
    assert np.allclose(tail[0], r["a"]["m"], rtol=1e-12, atol=1e-15) and np.allclose(tail[1], r["c"], rtol=1e-9, atol=1e-12)
    # a second launch gives the same bits
    b = Launch(c["y"], c["x1"], c["x2"], D)
    for x, y in zip(a.outputs(), b.outputs()):
        assert np.array_equal(x.bits(), y.bits()), "a second launch gives the same bits"


@pytest.mark.parametrize("Bh,C,T,D", [(3, 80, 64, 64), (2, 17, 128, 64)])
def test_a_row_does_not_depend_on_the_other_rows(Bh, C, T, D):
    """with N kept, a row's dy is a function of that row of y and of its own target"""
    c = reference(Bh, C, T, D)
    N = 2 * Bh
    a = Launch(c["y"], c["x1"], c["x2"], D).dy.bits()
    rs = np.random.RandomState(5)
    x = np.concatenate([c["x1"], c["x2"]], 0)
    for keep in (0, Bh - 1, Bh, N - 1):
        yn, xn = rs.uniform(0, 1, c["y"].shape).astype(F32), rs.uniform(0, 1, x.shape).astype(F32)
        yn[keep], xn[keep] = c["y"][keep], x[keep]
        b = Launch(yn, xn[:Bh], xn[Bh:], D).dy.bits()
        assert np.array_equal(a[keep], b[keep]), f"row {keep}: among other rows"
        assert not np.array_equal(a, b)


def test_gscale_scales_the_gradient():
    """the incoming gradient of the penalty multiplies the result before its one rounding: 2 is exact"""
    c = reference(1, 3, 24, 8)
    one = Launch(c["y"], c["x1"], c["x2"], 8, gscale=1.0)
    none = Launch(c["y"], c["x1"], c["x2"], 8, pen=False)                    # and without the penalty's second home
    two = Launch(c["y"], c["x1"], c["x2"], 8, gscale=2.0)
    assert np.array_equal(one.dy.bits(), none.dy.bits())
    assert np.array_equal((2.0 * one.dy.np()).view(np.uint32), two.dy.np().view(np.uint32))
    assert np.abs(one.dy.np()).max() > 0


@pytest.mark.parametrize("Bh,C,T,D", [(1, 3, 24, 8), (2, 17, 128, 64)])
def test_zero_weights_write_positive_zero(Bh, C, T, D):
    c = reference(Bh, C, T, D)
    y = c["y"].copy()
    y[1, 0, 3], y[0, C - 1, 1] = np.nan, np.inf
    a = Launch(y, c["x1"], c["x2"], D, weights=(0.0, 0.0), gscale=np.nan)
    assert (a.dy.bits() == 0).all(), "zero weights: every gradient element is +0.0"
    assert np.isnan(a.stats.np()).any()                  # the NaN is in the statistics, and stays there
    # one weight alone is not zero weights
    for w in ((0.0, 0.5), (0.5, 0.0)):
        assert np.abs(Launch(c["y"], c["x1"], c["x2"], D, weights=w).dy.np()).max() > 0


def test_refusals_leave_the_outputs_untouched():
    c = reference(1, 3, 24, 8)
    y, x1, x2, w = Pad(c["y"]), Pad(c["x1"]), Pad(c["x2"]), Pad(np.asarray(R.WEIGHTS, F32))
    tw = Buf(data=np.concatenate([R.twiddle(8).reshape(-1), np.zeros(512)]))
    Bh, C, T, D = 1, 3, 24, 8

    def call(fn, **kw):
        a = dict(y=y.ptr, x1=x1.ptr, x2=x2.ptr, Bh=Bh, C=C, T=T, D=D, floor=R.FLOOR, tw=tw.ptr, w=w.ptr, gs=None)
        outs = dict(stats=Buf((5,)), pen=Buf((1,)), ws=Buf((4096,), dtype=torch.float64), dy=Buf((2, 3, 24)))
        a.update({k: v.ptr for k, v in outs.items()})
        a.update(kw)
        if fn == "fwd":
            rc = L().dvae_msloss_fwd(a["y"], a["x1"], a["x2"], a["Bh"], a["C"], a["T"], a["D"], a["floor"], a["tw"], a["w"],
                                     a["stats"], a["pen"], a["ws"], st())
        else:
            rc = L().dvae_msloss_bwd(a["y"], a["x1"], a["x2"], a["Bh"], a["C"], a["T"], a["D"], a["floor"], a["tw"], a["w"],
                                     a["gs"], a["ws"], a["dy"], st())
        assert rc == EINVAL, (fn, kw, rc)
        guards(*outs.values())
        assert all(b.poisoned().all() for b in outs.values()), f"{fn} {kw}: a refused call wrote an output"
        return outs

    odd_ws = Buf((4097,), dtype=torch.float64)
    shapes = (dict(Bh=0), dict(Bh=-1), dict(C=0), dict(C=-3), dict(C=65536), dict(D=7), dict(D=6), dict(D=130), dict(D=0),
              dict(D=16), dict(T=20), dict(T=0), dict(T=4, D=8), dict(floor=0.0), dict(floor=-0.003), dict(floor=float("nan")),
              dict(floor=1e-200), dict(ws=odd_ws.ptr + 4), dict(tw=tw.ptr + 4))
    for kw in (dict(y=None), dict(x1=None), dict(x2=None), dict(tw=None), dict(w=None), dict(stats=None), dict(ws=None)) + shapes:
        call("fwd", **kw)
    for kw in (dict(y=None), dict(x1=None), dict(x2=None), dict(tw=None), dict(w=None), dict(dy=None), dict(ws=None)) + shapes:
        call("bwd", **kw)
    guards(odd_ws)
    assert odd_ws.poisoned().all()
    assert L().dvae_msloss_ws_bytes(0, 3) == -1 and L().dvae_msloss_ws_bytes(2, 0) == -1
    assert L().dvae_msloss_ws_bytes(2, 65536) == -1 and L().dvae_msloss_ws_bytes(6, 80) == 8 * ws_doubles(6, 80)
